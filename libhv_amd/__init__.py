"""libhv_amd -- MI355X-native WebSocket server receive path for libhv.

The product is the C-ABI shared library ``libhv_amd/libhvws.so`` (HIP kernels
for gfx950 + C/C++ host code, see include/*.h).  This Python module is a thin
ctypes binding used by the tests and by bench.py; it never computes anything
itself.  Loading fails loudly when the library has not been built: there is
no Python or CPU fallback for the receive path.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# $HVWS_LIB: another build of the library, for A/B runs on one box
LIB_PATH = os.environ.get("HVWS_LIB") or os.path.join(_HERE, "libhvws.so")

# enum websocket_flags (include/websocket_parser.h; reference http/websocket_parser.h:30-45)
WS_OP_CONTINUE, WS_OP_TEXT, WS_OP_BINARY = 0x0, 0x1, 0x2
WS_OP_CLOSE, WS_OP_PING, WS_OP_PONG = 0x8, 0x9, 0xA
WS_FIN, WS_HAS_MASK, WS_OP_MASK = 0x10, 0x20, 0x0F

I_HDR, I_BODY, I_END, I_START = 1 << 10, 1 << 11, 1 << 12, 1 << 13


class WsParser(ctypes.Structure):
    """struct websocket_parser (reference http/websocket_parser.h:50-62), 48 bytes."""

    _fields_ = [
        ("state", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("mask", ctypes.c_char * 4),
        ("mask_offset", ctypes.c_uint8),
        ("length", ctypes.c_size_t),
        ("require", ctypes.c_size_t),
        ("offset", ctypes.c_size_t),
        ("data", ctypes.c_void_p),
    ]

    def fields(self) -> tuple:
        """(state, flags, mask u32, mask_offset, length, require) -- offset excluded (Q12)."""
        return (
            self.state,
            self.flags,
            int.from_bytes(bytes(self.mask), "little"),
            self.mask_offset,
            self.length,
            self.require,
        )


class Segment(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64)]


class Frame(ctypes.Structure):
    _fields_ = [
        ("hdr_off", ctypes.c_int64),
        ("pay_off", ctypes.c_uint64),
        ("pay_len", ctypes.c_uint64),
        ("length", ctypes.c_uint64),
        ("key", ctypes.c_uint32),
        ("info", ctypes.c_uint32),
    ]


FRAME_DTYPE = np.dtype(
    [("hdr_off", "<i8"), ("pay_off", "<u8"), ("pay_len", "<u8"), ("length", "<u8"), ("key", "<u4"), ("info", "<u4")]
)
assert FRAME_DTYPE.itemsize == ctypes.sizeof(Frame) == 40
# hvws_msg / hvws_msg_state (include/hvws.h)
MSG_DTYPE = np.dtype(
    [("off", "<u8"), ("len", "<u8"), ("total", "<u8"), ("rec", "<u8"), ("seg", "<u4"), ("info", "<u4")]
)
MSG_STATE_DTYPE = np.dtype([("pending", "<u8"), ("opcode", "<u4"), ("open", "<u4")])
assert MSG_DTYPE.itemsize == 40 and MSG_STATE_DTYPE.itemsize == 16
MSG_END, MSG_CONT = 1 << 4, 1 << 5
# hvws_rfc_state and HVWS_M_CTL (hvws_messages_rfc)
RFC_STATE_DTYPE = np.dtype([("data", MSG_STATE_DTYPE), ("ctl", MSG_STATE_DTYPE), ("data_off", "<u8"), ("ctl_off", "<u8")])
assert RFC_STATE_DTYPE.itemsize == 48
M_CTL = 1 << 6
# hvws_tx_msg, HVWS_R_* and HVWS_RF_* (include/hvws.h)
TX_MSG_DTYPE = np.dtype([("off", "<u8"), ("len", "<u8"), ("flags", "<u4"), ("key", "<u4")])
assert TX_MSG_DTYPE.itemsize == 24
R_PONG, R_CLOSE, R_ECHO = 1, 2, 4
R_SERVER = R_PONG | R_CLOSE
RF_CLOSED, RF_DEFERRED = 1, 2
# HVWS_C_*, HVWS_CK_*, HVWS_CHECK_NONE and HVWS_RF_FAILED (hvws_check)
C_HEADER, C_SEQUENCE, C_CLOSE_BODY, C_CLOSE_UTF8, C_TEXT_UTF8, C_SIZE = 1, 2, 4, 8, 16, 32
C_ALL = 63
CK_OPEN, CK_FAILED = 1, 2
CHECK_NONE = (1 << 64) - 1
RF_FAILED = 4
# HVWS_FAN_* (hvws_fanout)
FAN_NONE, FAN_SELF = 0xFFFFFFFF, 1
# HVWS_BF_* (hvws_budget)
BF_OVER = 1
# HVWS_SUB_*, HVWS_SUBS_UNIQUE and hvws_sub_event (hvws_subs_update)
SUB_JOIN, SUB_LEAVE, SUB_DROP = 1, 2, 3
SUBS_UNIQUE = 1
SUBS_OVER = 2   # hvws_subs_update_routed only
SUB_EVENT_DTYPE = np.dtype([("op", "<u4"), ("topic", "<u4"), ("dest", "<u4")])
assert SUB_EVENT_DTYPE.itemsize == 12
# HVWS_ROUTE_*, HVWS_RK_* and HVWS_RT_BAD (hvws_route)
ROUTE_HDR_MAX = 12
# hvws_envelope
ENV_SENDER = 1
ENV_HDR_MAX = 23
# hvws_envelope_sequenced
SEQ_HDR_MAX = 45
RK_OTHER, RK_PUB, RK_SUB, RK_UNSUB, RK_BAD, RK_STOPPED = 0, 1, 2, 3, 4, 5
RT_BAD = 1
ROUTE_NONE = (1 << 64) - 1
# hvws_retained (hvws_retain)
RETAINED_DTYPE = np.dtype([("len", "<u8"), ("flags", "<u4"), ("set", "<u4")])
assert RETAINED_DTYPE.itemsize == 16
assert ctypes.sizeof(WsParser) == 48

MSG_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char), ctypes.c_size_t)

_lib: Optional[ctypes.CDLL] = None

# name -> (restype, argtypes)
_SIGS = {
    "hvws_device_count": (ctypes.c_int, []),
    "hvws_ctx_create": (ctypes.c_void_p, [ctypes.c_int]),
    "hvws_ctx_destroy": (None, [ctypes.c_void_p]),
    "hvws_last_error": (ctypes.c_char_p, []),
    "hvws_ctx_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_ctx_device": (ctypes.c_int, [ctypes.c_void_p]),
    "hvws_device_identity": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "hvws_dev_alloc": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_uint64]),
    "hvws_dev_free": (None, [ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_host_alloc": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_uint64]),
    "hvws_host_free": (None, [ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_h2d": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "hvws_d2h": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "hvws_d2d": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "hvws_memset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64]),
    "hvws_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "hvws_debug_stall": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "hvws_scan": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32],
    ),
    "hvws_unmask": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "hvws_step": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32],
    ),
    "hvws_step_resident": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32],
    ),
    "hvws_frame_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_get_frames": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "hvws_get_segment_frames": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_get_carry": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_last_times": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "hvws_step_times": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int]),
    "hvws_set_step_event_interval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "hvws_set_speculation": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "hvws_set_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "hvws_last_run_repairs": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_set_walk_verify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "hvws_last_scan_path": (ctypes.c_int, [ctypes.c_void_p]),
    "hvws_set_fast_bound": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64]),
    "hvws_stream_xor": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]),
    "hvws_rx_batch": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
         ctypes.c_int],
    ),
    "hvws_pipeline": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    ),
    "hvws_synth": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
         ctypes.POINTER(ctypes.c_uint64)],
    ),
    "hvws_digest": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_build_frames": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.POINTER(ctypes.c_uint64)],
    ),
    "hvws_encode_keys": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
    "hvws_last_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "hvws_utf8": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]),
    "hvws_get_utf8_words": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "hvws_get_utf8": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_utf8_tile": (ctypes.c_uint64, []),
    "hvws_utf8_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_messages": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p],
    ),
    "hvws_messages_joined": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
    "hvws_get_msg_carry": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_messages_rfc": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64],
    ),
    "hvws_get_rfc_state": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_msg_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_msg_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_get_messages": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "hvws_get_segment_messages": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_get_msg_state": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_messages_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_msg_tile": (ctypes.c_uint64, []),
    "hvws_send_messages": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p,
         ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
    ),
    "hvws_replies": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "hvws_replies_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_reply_count_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_reply_capacity": (ctypes.c_uint64, [ctypes.c_void_p]),
    "hvws_reply_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_get_replies": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    ),
    "hvws_get_segment_replies": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_get_reply_flags": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_check": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p]),
    "hvws_get_check": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    ),
    "hvws_check_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_replies_checked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "hvws_fanout": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)],
    ),
    "hvws_fanout_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_fanout_count_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_fanout_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_get_fanout": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    ),
    "hvws_get_dest_fanout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_route": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]),
    "hvws_route_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_route_topics_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_route_events_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_route_event_count_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_get_route": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64],
    ),
    "hvws_route_event_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_get_route_events": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "hvws_get_route_flags": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_get_route_totals": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_fanout_routed": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
         ctypes.POINTER(ctypes.c_uint64)],
    ),
    "hvws_retain": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32]
    ),
    "hvws_retain_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_retain_count_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_retain_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_get_retain": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64],
    ),
    "hvws_get_segment_retain": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_get_retain_totals": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_retain_tile": (ctypes.c_uint64, []),
    "hvws_envelope_bound": (ctypes.c_uint64, [ctypes.c_void_p]),
    "hvws_envelope_tile": (ctypes.c_uint32, []),
    "hvws_envelope": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]),
    "hvws_envelope_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_get_envelope": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "hvws_get_envelope_totals": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_fanout_enveloped": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
         ctypes.POINTER(ctypes.c_uint64)],
    ),
    "hvws_retain_enveloped": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32]
    ),
    "hvws_sequence": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "hvws_sequence_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_get_sequence": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "hvws_get_sequence_totals": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_envelope_sequenced_bound": (ctypes.c_uint64, [ctypes.c_void_p]),
    "hvws_envelope_sequenced": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]),
    "hvws_budget": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    ),
    "hvws_budget_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_budget_count_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "hvws_budget_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_get_budget": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    ),
    "hvws_get_dest_budget": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    ),
    "hvws_get_budget_totals": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_subs_update": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)],
    ),
    "hvws_subs_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "hvws_get_subs_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_subs_update_routed": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)],
    ),
    "hvws_get_subs_merged": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_get_subs_events": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "hvws_wsp_new": (ctypes.c_void_p, []),
    "hvws_wsp_free": (None, [ctypes.c_void_p]),
    "hvws_wsp_set_sink": (None, [ctypes.c_void_p, MSG_CB, ctypes.c_void_p]),
    "hvws_wsp_feed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "hvws_wsp_state": (None, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_wsp_feed_many": (
        ctypes.c_int,
        [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int,
         ctypes.POINTER(ctypes.c_int)],
    ),
    "hvws_host_register": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "hvws_host_unregister": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "hvws_rx_reads": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_uint32,
         ctypes.c_int],
    ),
    "hvws_feeder_new": (ctypes.c_void_p, []),
    "hvws_feeder_free": (None, [ctypes.c_void_p]),
    "hvws_feeder_flush": (ctypes.c_int, [ctypes.c_void_p]),
    "hvws_wsp_feeder_submit": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
         ctypes.c_int, ctypes.POINTER(ctypes.c_int)],
    ),
    "hvws_set_thread_device": (ctypes.c_int, [ctypes.c_int]),
    "hvws_thread_release": (None, []),
    "hvws_unmask_kernel_name": (ctypes.c_char_p, []),
    "hvws_unmask_kernel_name_for": (ctypes.c_char_p, [ctypes.c_uint64]),
    "hvws_run_kernel_name": (ctypes.c_char_p, []),
    "hvws_set_spec_min": (ctypes.c_uint64, [ctypes.c_uint64]),
    "hvws_set_sieve_min": (ctypes.c_uint64, [ctypes.c_uint64]),
    "hvws_set_table_checks": (ctypes.c_int, [ctypes.c_int]),
    "hvws_last_sieve": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_set_sieve_windows": (None, [ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_last_sieve_windows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_build_kernel_name": (ctypes.c_char_p, []),
    "hvws_last_build_kernel": (ctypes.c_char_p, [ctypes.c_void_p]),
    "hvws_last_build_uniform": (ctypes.c_int, [ctypes.c_void_p]),
    "hvws_span_begin": (ctypes.c_int, [ctypes.c_void_p]),
    "hvws_span_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "hvws_set_door": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "hvws_debug_dump": (ctypes.c_int, [ctypes.c_int]),
    "hvws_debug_backtraces": (ctypes.c_int, [ctypes.c_int]),
    "hvws_door_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_door_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_door_health": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_set_door_idle_us": (ctypes.c_uint64, [ctypes.c_uint64]),
    "hvws_door_stamps": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "hvws_set_small_batch_limit": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64]),
    "hvws_set_small_zero_copy": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "hvws_set_validation": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_uint32]),
    "hvws_set_unmask_variant": (ctypes.c_int, [ctypes.c_int]),
    # reference ABI (include/websocket_parser.h, include/wsdef.h)
    "websocket_parser_init": (None, [ctypes.c_void_p]),
    "websocket_parser_settings_init": (None, [ctypes.c_void_p]),
    "websocket_parser_execute": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "websocket_parser_decode": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "websocket_decode": (ctypes.c_uint8, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint8]),
    "websocket_calc_frame_size": (ctypes.c_size_t, [ctypes.c_uint32, ctypes.c_size_t]),
    "websocket_build_frame": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "ws_encode_key": (None, [ctypes.c_char_p, ctypes.c_char_p]),
    "ws_calc_frame_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_bool]),
    "ws_build_frame": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_bool, ctypes.c_int, ctypes.c_bool],
    ),
}

# C++ drop-in symbols (include/WebSocketParser.h)
CXX_SYMBOLS = (
    "_Z14hvws_feed_manyPKP15WebSocketParserPKPKcPKmiPi",
    "_Z18hvws_feeder_submitP11hvws_feederPKP15WebSocketParserPKPKcPKmiPi",
    "_ZN15WebSocketParserC1Ev",
    "_ZN15WebSocketParserD1Ev",
    "_ZN15WebSocketParser12FeedRecvDataEPKcm",
)


def lib() -> ctypes.CDLL:
    """Load libhvws.so (raises if it is missing: there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing -- build it with `make -C libhv_amd/csrc` "
            "(or __graft_entry__.build()); the receive path has no CPU fallback"
        )
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


class HvwsError(RuntimeError):
    pass


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise HvwsError(f"{what} failed ({rc}): {lib().hvws_last_error().decode(errors='replace')}")


def _ptr(a) -> int:
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a)


class DeviceBuffer:
    def __init__(self, eng: "Engine", nbytes: int):
        self.eng = eng
        self.nbytes = int(nbytes)
        self.ptr = lib().hvws_dev_alloc(eng.ctx, max(self.nbytes, 16))
        if not self.ptr:
            raise HvwsError(f"hvws_dev_alloc({nbytes}): {lib().hvws_last_error().decode()}")

    def free(self) -> None:
        if self.ptr:
            lib().hvws_dev_free(self.eng.ctx, self.ptr)
            self.ptr = None

    def upload(self, arr: np.ndarray, sync: bool = True) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check(lib().hvws_h2d(self.eng.ctx, self.ptr, arr.ctypes.data, arr.nbytes), "hvws_h2d")
        if sync:
            self.eng.sync()
        return self

    def download(self, nbytes: Optional[int] = None, dtype=np.uint8) -> np.ndarray:
        n = self.nbytes if nbytes is None else int(nbytes)
        out = np.empty(n, dtype=np.uint8)
        if n:
            _check(lib().hvws_d2h(self.eng.ctx, out.ctypes.data, self.ptr, n), "hvws_d2h")
            self.eng.sync()
        return out.view(dtype)


class Engine:
    """One hvws_ctx (device context + streams + frame tables)."""

    def __init__(self, device: int = 0):
        L = lib()
        self.ctx = L.hvws_ctx_create(device)
        if not self.ctx:
            raise HvwsError(f"hvws_ctx_create({device}): {L.hvws_last_error().decode()}")
        self.device = device

    def close(self) -> None:
        if self.ctx:
            lib().hvws_ctx_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr: np.ndarray, pad: int = 64) -> DeviceBuffer:
        arr = np.ascontiguousarray(arr)
        b = DeviceBuffer(self, arr.nbytes + pad)
        if arr.nbytes:
            b.upload(arr)
        return b

    def sync(self) -> None:
        _check(lib().hvws_sync(self.ctx), "hvws_sync")

    @staticmethod
    def _segs(segs: Sequence[Tuple[int, int]]):
        arr = (Segment * max(len(segs), 1))()
        for i, (o, n) in enumerate(segs):
            arr[i].off, arr[i].len = int(o), int(n)
        return arr

    @staticmethod
    def _carry(nseg: int, carry=None):
        arr = (WsParser * max(nseg, 1))()
        for i in range(nseg):
            if carry is not None and carry[i] is not None:
                ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(carry[i]), ctypes.sizeof(WsParser))
        return arr

    def scan(self, rx: DeviceBuffer, rx_len: int, segs, carry=None) -> int:
        s = self._segs(segs)
        c = self._carry(len(segs), carry)
        _check(lib().hvws_scan(self.ctx, rx.ptr, rx_len, s, c, len(segs)), "hvws_scan")
        return lib().hvws_frame_count(self.ctx)

    def unmask(self, rx: DeviceBuffer, rx_len: int) -> None:
        _check(lib().hvws_unmask(self.ctx, rx.ptr, rx_len), "hvws_unmask")

    def prepare(self, segs, carry=None) -> "Prepared":
        """Build the ctypes segment/carry tables once (for repeated steps)."""
        return Prepared(self._segs(segs), self._carry(len(segs), carry), len(segs))

    def step(self, rx: DeviceBuffer, rx_len: int, segs, carry=None) -> None:
        if isinstance(segs, Prepared):
            s, c, n = segs.segs, segs.carry, segs.n
        else:
            s, c, n = self._segs(segs), self._carry(len(segs), carry), len(segs)
        _check(lib().hvws_step(self.ctx, rx.ptr, rx_len, s, c, n), "hvws_step")

    def step_resident(self, rx: DeviceBuffer, rx_len: int, segs, carry=None) -> None:
        """hvws_step_resident: discovery overlaps the previous step's unmask."""
        if isinstance(segs, Prepared):
            s, c, n = segs.segs, segs.carry, segs.n
        else:
            s, c, n = self._segs(segs), self._carry(len(segs), carry), len(segs)
        _check(lib().hvws_step_resident(self.ctx, rx.ptr, rx_len, s, c, n), "hvws_step_resident")

    def frames(self) -> np.ndarray:
        n = lib().hvws_frame_count(self.ctx)
        out = np.zeros(max(n, 0), dtype=FRAME_DTYPE)
        if n > 0:
            _check(lib().hvws_get_frames(self.ctx, out.ctypes.data, 0, n), "hvws_get_frames")
        return out

    def segment_frames(self, nseg: int) -> Tuple[np.ndarray, np.ndarray]:
        first = np.zeros(nseg, np.uint64)
        cnt = np.zeros(nseg, np.uint64)
        _check(lib().hvws_get_segment_frames(self.ctx, first.ctypes.data, cnt.ctypes.data), "hvws_get_segment_frames")
        return first, cnt

    def carry(self, nseg: int):
        arr = (WsParser * max(nseg, 1))()
        started = (ctypes.c_int * max(nseg, 1))()
        _check(lib().hvws_get_carry(self.ctx, arr, started), "hvws_get_carry")
        return [arr[i] for i in range(nseg)], [started[i] for i in range(nseg)]

    def last_times(self) -> Tuple[float, float]:
        out = (ctypes.c_float * 2)()
        _check(lib().hvws_last_times(self.ctx, out), "hvws_last_times")
        return float(out[0]), float(out[1])

    def step_times(self, max_steps: int = 32) -> List[Tuple[float, float]]:
        """(scan ms, unmask ms) of the last max_steps steps (at most 32), oldest first."""
        out = (ctypes.c_float * (2 * max_steps))()
        n = lib().hvws_step_times(self.ctx, out, max_steps)
        if n < 0:
            _check(n, "hvws_step_times")
        return [(float(out[2 * i]), float(out[2 * i + 1])) for i in range(n)]

    def set_step_event_interval(self, every: int) -> int:
        """Timing events on every `every`-th step only (hvws_set_step_event_interval); returns the old interval."""
        r = lib().hvws_set_step_event_interval(self.ctx, every)
        if r < 0:
            _check(r, "hvws_set_step_event_interval")
        return r

    def stream_xor(self, buf: DeviceBuffer, n: int, pattern: int) -> None:
        _check(lib().hvws_stream_xor(self.ctx, buf.ptr, n, pattern), "hvws_stream_xor")

    def rx_batch(self, host: np.ndarray, segs, carry=None, unmask: bool = True):
        s = self._segs(segs)
        c = self._carry(len(segs), carry)
        _check(lib().hvws_rx_batch(self.ctx, host.ctypes.data, host.nbytes, s, c, len(segs), int(unmask)),
               "hvws_rx_batch")
        return [c[i] for i in range(len(segs))]

    def synth(self, buf: DeviceBuffer, buf_len: int, seed: int, plan: "DevicePlan", mode: int = 0) -> int:
        bad = ctypes.c_uint64(0)
        _check(
            lib().hvws_synth(self.ctx, buf.ptr, buf_len, seed, plan.n, plan.off.ptr, plan.flags.ptr, plan.mask.ptr,
                             plan.length.ptr, plan.text.ptr if plan.text else None, mode, ctypes.byref(bad)),
            "hvws_synth",
        )
        return int(bad.value)

    def build_frames(self, out: DeviceBuffer, out_cap: int, payload: Optional[DeviceBuffer], payload_len: int,
                     tx: "TxPlan", out_off: Optional[DeviceBuffer] = None) -> int:
        """Transmit side: websocket_build_frame for every frame of `tx` into
        `out` (back to back).  Returns the bytes written (the kernel runs
        asynchronously on the ctx stream)."""
        n = ctypes.c_uint64(0)
        _check(
            lib().hvws_build_frames(self.ctx, out.ptr, out_cap, payload.ptr if payload else None, payload_len,
                                    tx.pay_off.ptr, tx.length.ptr, tx.flags.ptr, tx.mask.ptr if tx.mask else None,
                                    tx.n, out_off.ptr if out_off else None, ctypes.byref(n)),
            "hvws_build_frames",
        )
        return int(n.value)

    def encode_keys(self, keys: Sequence[bytes]) -> List[bytes]:
        """Sec-WebSocket-Accept for every key (ws_encode_key, batched on the GPU)."""
        n = len(keys)
        if n == 0:
            return []
        lens = np.array([len(k) for k in keys], dtype=np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        blob = np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)
        dk, do, dl = self.to_device(blob), self.to_device(offs), self.to_device(lens)
        acc = self.alloc(32 * n)
        try:
            _check(lib().hvws_encode_keys(self.ctx, dk.ptr, do.ptr, dl.ptr, n, acc.ptr), "hvws_encode_keys")
            raw = acc.download(32 * n).tobytes()
        finally:
            for b in (dk, do, dl, acc):
                b.free()
        return [raw[32 * i:32 * i + 32] for i in range(n)]

    def last_kernel_ms(self) -> float:
        out = ctypes.c_float(0)
        _check(lib().hvws_last_kernel_ms(self.ctx, ctypes.byref(out)), "hvws_last_kernel_ms")
        return float(out.value)

    def utf8(self, rx: DeviceBuffer, rx_len: int, masked: bool, state_in=None) -> None:
        """hvws_utf8 over the last scan / step of rx: per-record transition words,
        then each segment's fold from state_in (one word per segment; None = 0)."""
        st = None
        if state_in is not None:
            st = np.ascontiguousarray(state_in, dtype=np.uint32)
        _check(lib().hvws_utf8(self.ctx, rx.ptr, rx_len, int(bool(masked)), st.ctypes.data if st is not None else None),
               "hvws_utf8")

    def utf8_words(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Transition words of the last utf8() call's records (all of them by default)."""
        if n is None:
            total = lib().hvws_utf8_count(self.ctx)
            if total < 0:
                _check(-2, "hvws_utf8_count")
            n = total - first
        out = np.zeros(max(n, 0), dtype=np.uint32)
        _check(lib().hvws_get_utf8_words(self.ctx, out.ctypes.data, first, max(n, 0)), "hvws_get_utf8_words")
        return out

    def utf8_result(self, nseg: int) -> Tuple[np.ndarray, np.ndarray]:
        """(state_out, bad) of the last utf8() call: per segment, the state word to
        carry into its next batch and the first rejecting record (U8_NONE if none)."""
        st = np.zeros(max(nseg, 1), dtype=np.uint32)
        bad = np.zeros(max(nseg, 1), dtype=np.uint64)
        _check(lib().hvws_get_utf8(self.ctx, st.ctypes.data, bad.ctypes.data), "hvws_get_utf8")
        return st[:nseg], bad[:nseg]

    def messages(self, rx: DeviceBuffer, rx_len: int, masked: bool, out: DeviceBuffer, out_cap: int,
                 state_in=None) -> None:
        """hvws_messages over the last scan / step of rx: the payload bytes, headers
        squeezed out (unmasked on the way when `masked`), into `out`, and the piece
        table.  state_in: one MSG_STATE_DTYPE entry per segment (None = all fresh)."""
        st = None
        if state_in is not None:
            st = np.ascontiguousarray(state_in, dtype=MSG_STATE_DTYPE)
        _check(lib().hvws_messages(self.ctx, rx.ptr, rx_len, int(bool(masked)), out.ptr, out_cap,
                                   st.ctypes.data if st is not None else None), "hvws_messages")

    def messages_joined(self, rx: DeviceBuffer, rx_len: int, masked: bool, out: DeviceBuffer, out_cap: int,
                        state_in=None, prev=None, prev_len: int = 0, prev_off=None) -> None:
        """hvws_messages_joined: messages() with each segment's state_in.pending
        carried bytes, prev[prev_off[s] ..) of the previous call's output, copied
        ahead of the segment's payload bytes, so that every M_END piece is a whole
        message in `out`.  prev: a DeviceBuffer or a device address; prev_off: one
        offset per segment (both None = nothing pending)."""
        st = None
        if state_in is not None:
            st = np.ascontiguousarray(state_in, dtype=MSG_STATE_DTYPE)
        po = None
        if prev_off is not None:
            po = np.ascontiguousarray(prev_off, dtype=np.uint64)
        pp = prev.ptr if hasattr(prev, "ptr") else prev
        _check(lib().hvws_messages_joined(self.ctx, rx.ptr, rx_len, int(bool(masked)), out.ptr, out_cap,
                                          st.ctypes.data if st is not None else None, pp, prev_len,
                                          po.ctypes.data if po is not None else None), "hvws_messages_joined")

    def msg_carry(self, nseg: int) -> np.ndarray:
        """Per segment of the last messages_joined() call, the offset in its output
        of the trailing open piece: the connection's prev_off in its next batch."""
        out = np.zeros(max(nseg, 1), dtype=np.uint64)
        _check(lib().hvws_get_msg_carry(self.ctx, out.ctypes.data), "hvws_get_msg_carry")
        return out[:nseg]

    def messages_rfc(self, rx: DeviceBuffer, rx_len: int, masked: bool, out: DeviceBuffer, out_cap: int,
                     state_in=None, prev=None, prev_len: int = 0) -> None:
        """hvws_messages_rfc: messages_joined() with RFC 6455's message rule -- each
        connection's control frames are messages of their own (M_CTL pieces, behind
        the connection's data pieces) and no longer land in the fragmented data
        message they interrupt.  state_in: one RFC_STATE_DTYPE entry per segment,
        its offsets pointing into prev (None = all fresh)."""
        st = None
        if state_in is not None:
            st = np.ascontiguousarray(state_in, dtype=RFC_STATE_DTYPE)
        pp = prev.ptr if hasattr(prev, "ptr") else prev
        _check(lib().hvws_messages_rfc(self.ctx, rx.ptr, rx_len, int(bool(masked)), out.ptr, out_cap,
                                       st.ctypes.data if st is not None else None, pp, prev_len), "hvws_messages_rfc")

    def rfc_state(self, nseg: int) -> np.ndarray:
        """Per segment of the last messages_rfc() call, the state to carry into the
        connection's next batch (RFC_STATE_DTYPE), offsets into that call's output."""
        out = np.zeros(max(nseg, 1), dtype=RFC_STATE_DTYPE)
        _check(lib().hvws_get_rfc_state(self.ctx, out.ctypes.data), "hvws_get_rfc_state")
        return out[:nseg]

    def message_table(self) -> np.ndarray:
        """The pieces of the last messages() call (MSG_DTYPE)."""
        n = lib().hvws_msg_count(self.ctx)
        if n < 0:
            _check(-2, "hvws_msg_count")
        out = np.zeros(n, dtype=MSG_DTYPE)
        _check(lib().hvws_get_messages(self.ctx, out.ctypes.data, 0, n), "hvws_get_messages")
        return out

    def segment_messages(self, nseg: int) -> Tuple[np.ndarray, np.ndarray]:
        """(first piece, piece count) per segment of the last messages() call."""
        first = np.zeros(max(nseg, 1), np.uint64)
        cnt = np.zeros(max(nseg, 1), np.uint64)
        _check(lib().hvws_get_segment_messages(self.ctx, first.ctypes.data, cnt.ctypes.data),
               "hvws_get_segment_messages")
        return first[:nseg], cnt[:nseg]

    def msg_state(self, nseg: int) -> np.ndarray:
        """Per segment, the state to carry into the connection's next batch (MSG_STATE_DTYPE)."""
        out = np.zeros(max(nseg, 1), dtype=MSG_STATE_DTYPE)
        _check(lib().hvws_get_msg_state(self.ctx, out.ctypes.data), "hvws_get_msg_state")
        return out[:nseg]

    def msg_bytes(self) -> int:
        """Bytes the last messages() call wrote to its output."""
        n = ctypes.c_uint64(0)
        _check(lib().hvws_msg_bytes(self.ctx, ctypes.byref(n)), "hvws_msg_bytes")
        return int(n.value)

    def send_messages(self, out: DeviceBuffer, out_cap: int, payload, payload_len: int, msgs, n: int,
                      d_n=None, fragment: int = 0, masked: bool = False,
                      msg_off: Optional[DeviceBuffer] = None) -> Tuple[int, int]:
        """hvws_send_messages: WebSocketChannel::send for the first min(*d_n, n)
        entries of the device table `msgs` (TX_MSG_DTYPE) over `payload`.  payload,
        msgs and d_n are DeviceBuffers or device addresses (replies_device()).
        Returns (bytes, frames); the build runs asynchronously on the ctx stream."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        nbytes, nfr = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = lib().hvws_send_messages(self.ctx, dev(out), out_cap, dev(payload), payload_len, dev(msgs), n, dev(d_n),
                                      fragment, int(bool(masked)), dev(msg_off), ctypes.byref(nbytes),
                                      ctypes.byref(nfr))
        self.last_send_len = int(nbytes.value)   # set even when the call fails for out_cap
        _check(rc, "hvws_send_messages")
        return int(nbytes.value), int(nfr.value)

    def replies(self, policy: int, closed_in=None) -> None:
        """hvws_replies over the last messages() call: the server's onMessage
        dispatch as a reply table on the device.  closed_in: one byte per segment."""
        ci = None
        if closed_in is not None:
            ci = np.ascontiguousarray(closed_in, dtype=np.uint8)
        _check(lib().hvws_replies(self.ctx, policy, ci.ctypes.data if ci is not None else None), "hvws_replies")

    def replies_device(self) -> Tuple[int, int, int]:
        """(table address, count word address, table capacity): msgs, d_n and n of
        send_messages for the last replies() call; no wait."""
        L = lib()
        return L.hvws_replies_device(self.ctx), L.hvws_reply_count_device(self.ctx), L.hvws_reply_capacity(self.ctx)

    def reply_table(self) -> Tuple[np.ndarray, np.ndarray]:
        """(replies [TX_MSG_DTYPE], the piece each answers) of the last replies() call."""
        n = lib().hvws_reply_count(self.ctx)
        if n < 0:
            _check(-2, "hvws_reply_count")
        out = np.zeros(n, dtype=TX_MSG_DTYPE)
        piece = np.zeros(n, dtype=np.uint64)
        _check(lib().hvws_get_replies(self.ctx, out.ctypes.data, piece.ctypes.data, 0, n), "hvws_get_replies")
        return out, piece

    def segment_replies(self, nseg: int) -> Tuple[np.ndarray, np.ndarray]:
        """(first reply, reply count) per segment of the last replies() call."""
        first = np.zeros(max(nseg, 1), np.uint64)
        cnt = np.zeros(max(nseg, 1), np.uint64)
        _check(lib().hvws_get_segment_replies(self.ctx, first.ctypes.data, cnt.ctypes.data),
               "hvws_get_segment_replies")
        return first[:nseg], cnt[:nseg]

    def reply_flags(self, nseg: int) -> np.ndarray:
        """RF_* per segment of the last replies() call."""
        out = np.zeros(max(nseg, 1), np.uint8)
        _check(lib().hvws_get_reply_flags(self.ctx, out.ctypes.data), "hvws_get_reply_flags")
        return out[:nseg]

    def check(self, classes: int = C_ALL, max_message: int = 0, state_in=None) -> None:
        """hvws_check over the last messages_rfc() call: which connections broke
        the protocol (C_* classes), where and with which close code.  state_in:
        one word per segment (CK_OPEN | CK_FAILED; None = all fresh).  No wait."""
        st = None
        if state_in is not None:
            st = np.ascontiguousarray(state_in, dtype=np.uint32)
        _check(lib().hvws_check(self.ctx, classes, max_message, st.ctypes.data if st is not None else None),
               "hvws_check")

    def check_result(self, nseg: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(state_out, fail_rec, why, code) per segment of the last check() call:
        the word to carry into the connection's next batch, the first violating
        record (CHECK_NONE if none), the classes violated there, the close code."""
        st = np.zeros(max(nseg, 1), dtype=np.uint32)
        fail = np.zeros(max(nseg, 1), dtype=np.uint64)
        why = np.zeros(max(nseg, 1), dtype=np.uint32)
        code = np.zeros(max(nseg, 1), dtype=np.uint16)
        _check(lib().hvws_get_check(self.ctx, st.ctypes.data, fail.ctypes.data, why.ctypes.data, code.ctypes.data),
               "hvws_get_check")
        return st[:nseg], fail[:nseg], why[:nseg], code[:nseg]

    def replies_checked(self, policy: int, closed_in=None) -> None:
        """hvws_replies_checked: replies() with the last check()'s fail_rec as a
        second limit -- nothing at or after a connection's failing record is
        answered, and the connection's flags carry RF_FAILED | RF_CLOSED."""
        ci = None
        if closed_in is not None:
            ci = np.ascontiguousarray(closed_in, dtype=np.uint8)
        _check(lib().hvws_replies_checked(self.ctx, policy, ci.ctypes.data if ci is not None else None),
               "hvws_replies_checked")

    def fanout(self, topic_first, member, ntopics: int, nmember: int, ndest: int, pub, dest_of, flags: int = 0,
               max_deliveries: int = (1 << 64) - 1) -> int:
        """hvws_fanout over the last replies() / replies_checked() call: its reply
        table through the subscription table (topic_first, member: DeviceBuffers or
        device addresses) into a delivery table ordered by destination.  pub: the
        topic each segment publishes to (FAN_NONE: none; None = all none);
        dest_of: each segment's own destination id.  Returns the deliveries;
        last_deliveries holds them even when the call fails for max_deliveries."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        pb = np.ascontiguousarray(pub, dtype=np.uint32) if pub is not None else None
        do = np.ascontiguousarray(dest_of, dtype=np.uint32) if dest_of is not None else None
        n = ctypes.c_uint64(0)
        rc = lib().hvws_fanout(self.ctx, dev(topic_first), dev(member), ntopics, nmember, ndest,
                               pb.ctypes.data if pb is not None and pb.size else None,
                               do.ctypes.data if do is not None else None, flags, max_deliveries, ctypes.byref(n))
        self.last_deliveries = int(n.value)
        _check(rc, "hvws_fanout")
        return int(n.value)

    def fanout_device(self) -> Tuple[int, int, int]:
        """(table address, count word address, deliveries): msgs, d_n and n of
        send_messages for the last fanout() call; (None, None, 0) when there is none."""
        L = lib()
        n = L.hvws_fanout_count(self.ctx)
        return L.hvws_fanout_device(self.ctx), L.hvws_fanout_count_device(self.ctx), max(int(n), 0)

    def fanout_table(self) -> Tuple[np.ndarray, np.ndarray]:
        """(deliveries [TX_MSG_DTYPE], the reply each carries) of the last fanout() call."""
        n = lib().hvws_fanout_count(self.ctx)
        if n < 0:
            _check(-2, "hvws_fanout_count")
        out = np.zeros(n, dtype=TX_MSG_DTYPE)
        reply = np.zeros(n, dtype=np.uint64)
        _check(lib().hvws_get_fanout(self.ctx, out.ctypes.data, reply.ctypes.data, 0, n), "hvws_get_fanout")
        return out, reply

    def dest_fanout(self, ndest: int) -> Tuple[np.ndarray, np.ndarray]:
        """(first delivery, delivery count) per destination of the last fanout() call."""
        first = np.zeros(max(ndest, 1), np.uint64)
        cnt = np.zeros(max(ndest, 1), np.uint64)
        _check(lib().hvws_get_dest_fanout(self.ctx, first.ctypes.data, cnt.ctypes.data), "hvws_get_dest_fanout")
        return first[:ndest], cnt[:ndest]

    def route(self, ntopics: int, ndest: int, dest_of) -> None:
        """hvws_route over the last replies() / replies_checked() call: every TEXT /
        BINARY reply classified by its command header ('P' / 'S' / 'U', a decimal
        topic id, LF) into a topic per reply, the rows with the header trimmed off
        and the join / leave events.  dest_of: each segment's own destination id.
        No wait."""
        do = np.ascontiguousarray(dest_of, dtype=np.uint32) if dest_of is not None else None
        _check(lib().hvws_route(self.ctx, ntopics, ndest, do.ctypes.data if do is not None else None), "hvws_route")

    def route_table(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(routed rows [TX_MSG_DTYPE], topic, kind RK_*) per reply of the last route() call."""
        L = lib()
        if not L.hvws_route_device(self.ctx):
            _check(-2, "hvws_get_route")
        n = L.hvws_reply_count(self.ctx)
        if n < 0:
            _check(-2, "hvws_reply_count")
        rows = np.zeros(n, dtype=TX_MSG_DTYPE)
        topic = np.zeros(n, dtype=np.uint32)
        kind = np.zeros(n, dtype=np.uint8)
        _check(L.hvws_get_route(self.ctx, rows.ctypes.data, topic.ctypes.data, kind.ctypes.data, 0, n), "hvws_get_route")
        return rows, topic, kind

    def route_events(self) -> np.ndarray:
        """The join / leave events [SUB_EVENT_DTYPE] of the last route() call, in
        reply order: the events argument of subs_update()."""
        n = lib().hvws_route_event_count(self.ctx)
        if n < 0:
            _check(-2, "hvws_route_event_count")
        out = np.zeros(n, dtype=SUB_EVENT_DTYPE)
        _check(lib().hvws_get_route_events(self.ctx, out.ctypes.data, 0, n), "hvws_get_route_events")
        return out

    def route_flags(self, nseg: int) -> Tuple[np.ndarray, np.ndarray]:
        """(RT_* flags, first malformed reply or ROUTE_NONE) per segment of the last route() call."""
        flags = np.zeros(max(nseg, 1), np.uint8)
        bad = np.zeros(max(nseg, 1), np.uint64)
        _check(lib().hvws_get_route_flags(self.ctx, flags.ctypes.data, bad.ctypes.data), "hvws_get_route_flags")
        return flags[:nseg], bad[:nseg]

    def route_totals(self) -> Tuple[int, int, int, int]:
        """(publications, subscribes, unsubscribes, bad + stopped) of the last route() call."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().hvws_get_route_totals(self.ctx, out), "hvws_get_route_totals")
        return tuple(int(x) for x in out)

    def fanout_routed(self, topic_first, member, nmember: int, flags: int = 0,
                      max_deliveries: int = (1 << 64) - 1) -> int:
        """hvws_fanout_routed: fanout() with the topic per reply, the rows, ntopics,
        ndest and dest_of of the last route() call.  Returns the deliveries;
        last_deliveries holds them even when the call fails for max_deliveries.
        fanout_table(), dest_fanout(), budget() and send_messages() follow as
        they follow fanout()."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        n = ctypes.c_uint64(0)
        rc = lib().hvws_fanout_routed(self.ctx, dev(topic_first), dev(member), nmember, flags, max_deliveries,
                                      ctypes.byref(n))
        self.last_deliveries = int(n.value)
        _check(rc, "hvws_fanout_routed")
        return int(n.value)

    def retain(self, store, slot: int, ret, flags: int = 0) -> None:
        """hvws_retain behind the last route() call: each topic's last publication
        of the turn into the caller's store (store: ntopics slots of `slot` bytes;
        ret: ntopics RETAINED_DTYPE entries; DeviceBuffers or device addresses,
        kept across turns), and a snapshot row per subscribe of the turn whose
        topic holds a message afterwards.  No wait."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        _check(lib().hvws_retain(self.ctx, dev(store), slot, dev(ret), flags), "hvws_retain")

    def retain_device(self) -> Tuple[int, int, int]:
        """(table address, count word address, the reply capacity): msgs, d_n and n
        of the send_messages() that sends the last retain() call's snapshot from
        the store; (None, None, 0) when there is none."""
        L = lib()
        t, d_n = L.hvws_retain_device(self.ctx), L.hvws_retain_count_device(self.ctx)
        return t, d_n, int(L.hvws_reply_capacity(self.ctx)) if t else 0

    def retain_table(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(snapshot rows [TX_MSG_DTYPE] over the store, the topic, the SUB reply)
        of the last retain() call, in reply order."""
        n = lib().hvws_retain_count(self.ctx)
        if n < 0:
            _check(-2, "hvws_retain_count")
        rows = np.zeros(n, dtype=TX_MSG_DTYPE)
        topic = np.zeros(n, dtype=np.uint32)
        reply = np.zeros(n, dtype=np.uint64)
        _check(lib().hvws_get_retain(self.ctx, rows.ctypes.data, topic.ctypes.data, reply.ctypes.data, 0, n),
               "hvws_get_retain")
        return rows, topic, reply

    def segment_retain(self, nseg: int) -> Tuple[np.ndarray, np.ndarray]:
        """(first snapshot row, row count) per segment of the last retain() call."""
        first = np.zeros(max(nseg, 1), np.uint64)
        cnt = np.zeros(max(nseg, 1), np.uint64)
        _check(lib().hvws_get_segment_retain(self.ctx, first.ctypes.data, cnt.ctypes.data), "hvws_get_segment_retain")
        return first[:nseg], cnt[:nseg]

    def retain_totals(self) -> Tuple[int, int, int, int, int]:
        """(topics stored, cleared by an empty publication, cleared by an oversize
        one, bytes copied, snapshot rows) of the last retain() call."""
        out = (ctypes.c_uint64 * 5)()
        _check(lib().hvws_get_retain_totals(self.ctx, out), "hvws_get_retain_totals")
        return tuple(int(x) for x in out)

    def envelope_bound(self) -> int:
        """hvws_envelope_bound: the env_cap envelope() needs behind the last route()
        call (0: there is none).  No wait."""
        return int(lib().hvws_envelope_bound(self.ctx))

    def envelope(self, env, env_cap: int, flags: int = 0) -> None:
        """hvws_envelope behind the last route() call: every reply's outgoing bytes
        written once into env (a DeviceBuffer or a device address, 16-byte
        aligned, env_cap >= envelope_bound() bytes), publications behind the line
        'M<topic>\n' (ENV_SENDER: 'M<topic> <sender>\n'), each reply 16-byte
        aligned.  No wait."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        _check(lib().hvws_envelope(self.ctx, dev(env), env_cap, flags), "hvws_envelope")

    def envelope_device(self) -> Tuple[int, int, int]:
        """(table address, count word address, the reply capacity): msgs, d_n and n
        of a send_messages() over the last envelope() call's rows; (None, None, 0)
        when there is none."""
        L = lib()
        t = L.hvws_envelope_device(self.ctx)
        return (t, L.hvws_reply_count_device(self.ctx), int(L.hvws_reply_capacity(self.ctx))) if t else (None, None, 0)

    def envelope_table(self) -> np.ndarray:
        """The enveloped rows [TX_MSG_DTYPE] over env, one per reply of the last
        envelope() call."""
        L = lib()
        if not L.hvws_envelope_device(self.ctx):
            _check(-2, "hvws_get_envelope")
        n = L.hvws_reply_count(self.ctx)
        if n < 0:
            _check(-2, "hvws_reply_count")
        rows = np.zeros(n, dtype=TX_MSG_DTYPE)
        _check(L.hvws_get_envelope(self.ctx, rows.ctypes.data, 0, n), "hvws_get_envelope")
        return rows

    def envelope_totals(self) -> Tuple[int, int, int, int]:
        """(enveloped publications, replies copied verbatim, bytes written, bytes of
        env spanned) of the last envelope() call."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().hvws_get_envelope_totals(self.ctx, out), "hvws_get_envelope_totals")
        return tuple(int(x) for x in out)

    def fanout_enveloped(self, topic_first, member, nmember: int, flags: int = 0,
                         max_deliveries: int = (1 << 64) - 1) -> int:
        """hvws_fanout_enveloped: fanout_routed() delivering the rows of the last
        envelope() call.  The send_messages() that follows takes env and env_cap
        as its payload."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        n = ctypes.c_uint64(0)
        rc = lib().hvws_fanout_enveloped(self.ctx, dev(topic_first), dev(member), nmember, flags, max_deliveries,
                                         ctypes.byref(n))
        self.last_deliveries = int(n.value)
        _check(rc, "hvws_fanout_enveloped")
        return int(n.value)

    def retain_enveloped(self, store, slot: int, ret, flags: int = 0) -> None:
        """hvws_retain_enveloped: retain() keeping the last envelope() call's bytes,
        envelope and body, so that a snapshot names its topic.  No wait."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        _check(lib().hvws_retain_enveloped(self.ctx, dev(store), slot, dev(ret), flags), "hvws_retain_enveloped")

    def sequence(self, seq_buf, flags: int = 0) -> None:
        """hvws_sequence behind the last route() call: every publication of the turn
        gets the next number of its topic, in table order.  seq_buf: the counters,
        ntopics words of 8 bytes in device memory (a DeviceBuffer or a device
        address), kept across turns; seq_buf[t] is the last number given out in
        topic t.  A turn is numbered once.  No wait."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        _check(lib().hvws_sequence(self.ctx, dev(seq_buf), flags), "hvws_sequence")

    def sequence_table(self) -> np.ndarray:
        """The number per reply (uint64; 0 where the reply is no publication) of the
        last sequence() call."""
        L = lib()
        if not L.hvws_sequence_device(self.ctx):
            _check(-2, "hvws_get_sequence")
        n = L.hvws_reply_count(self.ctx)
        if n < 0:
            _check(-2, "hvws_reply_count")
        seq = np.zeros(n, dtype=np.uint64)
        _check(L.hvws_get_sequence(self.ctx, seq.ctypes.data, 0, n), "hvws_get_sequence")
        return seq

    def sequence_totals(self) -> Tuple[int, int]:
        """(publications numbered, distinct topics published to) of the last
        sequence() call."""
        out = (ctypes.c_uint64 * 2)()
        _check(lib().hvws_get_sequence_totals(self.ctx, out), "hvws_get_sequence_totals")
        return tuple(int(x) for x in out)

    def envelope_sequenced_bound(self) -> int:
        """hvws_envelope_sequenced_bound: the env_cap envelope_sequenced() needs
        behind the last route() call (0: there is none).  No wait."""
        return int(lib().hvws_envelope_sequenced_bound(self.ctx))

    def envelope_sequenced(self, env, env_cap: int, flags: int = 0) -> None:
        """hvws_envelope_sequenced behind the last sequence() call: envelope() with
        the line 'M<topic> #<seq>\n' (ENV_SENDER: 'M<topic> <sender> #<seq>\n').
        env_cap >= envelope_sequenced_bound().  Fills envelope()'s tables:
        envelope_table(), fanout_enveloped() and retain_enveloped() follow.  No
        wait."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        _check(lib().hvws_envelope_sequenced(self.ctx, dev(env), env_cap, flags), "hvws_envelope_sequenced")

    def budget(self, budget, budget_all: int = (1 << 64) - 1, fragment: int = 0, masked: bool = False) -> None:
        """hvws_budget over the last fanout() call: every destination's deliveries
        cut at its byte budget.  budget: ndest words of 8 bytes in device memory (a
        DeviceBuffer or a device address), or None: budget_all for every
        destination.  fragment / masked: those of the send_messages() that
        follows.  No wait."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        _check(lib().hvws_budget(self.ctx, dev(budget), budget_all, fragment, int(masked)), "hvws_budget")

    def budget_device(self) -> Tuple[int, int, int]:
        """(table address, count word address, the fan-out's deliveries): msgs, d_n
        and n of send_messages for the last budget() call; (None, None, 0) when
        there is none.  No wait."""
        L = lib()
        table, d_n = L.hvws_budget_device(self.ctx), L.hvws_budget_count_device(self.ctx)
        return table, d_n, max(int(L.hvws_fanout_count(self.ctx)), 0) if table else 0

    def budget_table(self) -> Tuple[np.ndarray, np.ndarray]:
        """(kept deliveries [TX_MSG_DTYPE], the reply each carries) of the last budget() call."""
        n = lib().hvws_budget_count(self.ctx)
        if n < 0:
            _check(-2, "hvws_budget_count")
        out = np.zeros(n, dtype=TX_MSG_DTYPE)
        reply = np.zeros(n, dtype=np.uint64)
        _check(lib().hvws_get_budget(self.ctx, out.ctypes.data, reply.ctypes.data, 0, n), "hvws_get_budget")
        return out, reply

    def dest_budget(self, ndest: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(first kept delivery, kept count, byte_off [ndest + 1], BF_* flags) per
        destination of the last budget() call."""
        first = np.zeros(max(ndest, 1), np.uint64)
        cnt = np.zeros(max(ndest, 1), np.uint64)
        off = np.zeros(ndest + 1, np.uint64)
        flags = np.zeros(max(ndest, 1), np.uint8)
        _check(lib().hvws_get_dest_budget(self.ctx, first.ctypes.data, cnt.ctypes.data, off.ctypes.data,
                                          flags.ctypes.data), "hvws_get_dest_budget")
        return first[:ndest], cnt[:ndest], off, flags[:ndest]

    def budget_totals(self) -> Tuple[int, int, int, int]:
        """(kept deliveries, kept bytes, dropped deliveries, destinations over) of
        the last budget() call; the kept bytes are the exact length of the send."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().hvws_get_budget_totals(self.ctx, out), "hvws_get_budget_totals")
        return tuple(int(x) for x in out)

    def subs_update(self, topic_first, member, ntopics: int, nmember: int, ndest: int, events, dest_of,
                    topic_first_out, member_out, member_cap: int, flags: int = 0) -> int:
        """hvws_subs_update: the next subscription table (topic_first_out,
        member_out: DeviceBuffers or device addresses, member_cap ids) from the
        current one (topic_first, member), the events (SUB_EVENT_DTYPE, or
        (op, topic, dest) triples) and, with dest_of (one id per segment of the
        last reply call; None: no implicit drops), the connections that call
        closed.  Returns the new nmember; last_subs_nmember holds it even when
        the call fails for member_cap."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        if isinstance(events, np.ndarray) and events.dtype == SUB_EVENT_DTYPE:
            ev = np.ascontiguousarray(events)
        else:
            ev = np.array([tuple(e) for e in events], dtype=SUB_EVENT_DTYPE)
        do = np.ascontiguousarray(dest_of, dtype=np.uint32) if dest_of is not None else None
        n = ctypes.c_uint64(0)
        rc = lib().hvws_subs_update(self.ctx, dev(topic_first), dev(member), ntopics, nmember, ndest,
                                    ev.ctypes.data if ev.size else None, ev.size,
                                    do.ctypes.data if do is not None else None, flags, dev(topic_first_out),
                                    dev(member_out), member_cap, ctypes.byref(n))
        self.last_subs_nmember = int(n.value)
        _check(rc, "hvws_subs_update")
        return int(n.value)

    def subs_counts(self) -> Tuple[int, int, int, int]:
        """(old listings kept, listings added, old listings removed, destinations
        dropped as closed) of the last subs_update() call."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().hvws_get_subs_counts(self.ctx, out), "hvws_get_subs_counts")
        return tuple(int(x) for x in out)

    def subs_update_routed(self, topic_first, member, nmember: int, events, topic_first_out, member_out,
                           member_cap: int, flags: int = 0) -> int:
        """hvws_subs_update_routed: subs_update() with the events merged on the
        device -- the last route() call's events, a DROP per connection the reply
        call closed or the route found malformed, with SUBS_OVER a DROP per
        destination the last budget() cut, then `events` (the host's own; may be
        empty).  ntopics, ndest and dest_of are the route call's.  Returns the new
        nmember; last_subs_nmember holds it even when the call fails for
        member_cap."""
        dev = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        if isinstance(events, np.ndarray) and events.dtype == SUB_EVENT_DTYPE:
            ev = np.ascontiguousarray(events)
        else:
            ev = np.array([tuple(e) for e in events], dtype=SUB_EVENT_DTYPE)
        n = ctypes.c_uint64(0)
        rc = lib().hvws_subs_update_routed(self.ctx, dev(topic_first), dev(member), nmember,
                                           ev.ctypes.data if ev.size else None, ev.size, flags, dev(topic_first_out),
                                           dev(member_out), member_cap, ctypes.byref(n))
        self.last_subs_nmember = int(n.value)
        _check(rc, "hvws_subs_update_routed")
        return int(n.value)

    def subs_merged(self) -> Tuple[int, int, int, int]:
        """(route events, connection drops, OVER drops, host events) of the last
        subs_update_routed() call: the four parts of its merged event array."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().hvws_get_subs_merged(self.ctx, out), "hvws_get_subs_merged")
        return tuple(int(x) for x in out)

    def subs_events(self) -> np.ndarray:
        """The merged event array [SUB_EVENT_DTYPE] of the last subs_update_routed() call."""
        n = sum(self.subs_merged())
        out = np.zeros(n, dtype=SUB_EVENT_DTYPE)
        _check(lib().hvws_get_subs_events(self.ctx, out.ctypes.data, 0, n), "hvws_get_subs_events")
        return out

    def digest(self, buf: DeviceBuffer, n: int) -> int:
        out = ctypes.c_uint64(0)
        _check(lib().hvws_digest(self.ctx, buf.ptr, n, ctypes.byref(out)), "hvws_digest")
        return int(out.value)


class Prepared:
    def __init__(self, segs, carry, n):
        self.segs, self.carry, self.n = segs, carry, n


class DevicePlan:
    """A synthetic batch plan resident on the device (see libhv_amd.synth)."""

    def __init__(self, eng: Engine, plan):
        self.n = len(plan.length)
        self.off = eng.to_device(plan.frame_off.astype(np.uint64))
        self.flags = eng.to_device(plan.flags.astype(np.uint8))
        self.mask = eng.to_device(plan.mask.astype(np.uint32))
        self.length = eng.to_device(plan.length.astype(np.uint64))
        self.text = eng.to_device(plan.text.astype(np.uint8)) if plan.text is not None else None

    def free(self):
        for b in (self.off, self.flags, self.mask, self.length, self.text):
            if b is not None:
                b.free()


class TxPlan:
    """Outgoing-frame tables on the device for Engine.build_frames: frame i is
    websocket_build_frame(flags[i], mask[i], payload + pay_off[i], length[i])."""

    def __init__(self, eng: Engine, pay_off, length, flags, mask=None):
        self.n = len(length)
        self.pay_off = eng.to_device(np.asarray(pay_off, dtype=np.uint64))
        self.length = eng.to_device(np.asarray(length, dtype=np.uint64))
        self.flags = eng.to_device(np.asarray(flags, dtype=np.uint8))
        self.mask = eng.to_device(np.asarray(mask, dtype=np.uint32)) if mask is not None else None

    def free(self):
        for b in (self.pay_off, self.length, self.flags, self.mask):
            if b is not None:
                b.free()


def device_count() -> int:
    return lib().hvws_device_count()


def device_identity(device: int) -> tuple:
    """(PCI bus id, the device hipGetDevice reports once `device` is
    selected): which physical card a rank ran on."""
    buf = ctypes.create_string_buffer(64)
    cur = ctypes.c_int(-1)
    _check(lib().hvws_device_identity(device, buf, 64, ctypes.byref(cur)), "hvws_device_identity")
    return buf.value.decode(), int(cur.value)

