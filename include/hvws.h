/*
 * hvws.h -- batch / device-resident C ABI of the MI355X WebSocket receive
 * engine (libhv_amd/libhvws.so).  New entry points; the reference has no
 * batch API.  What each one stands in for:
 *
 *   hvws_scan    websocket_parser_execute's header state machine
 *                (reference http/websocket_parser.c:53-171) run over many
 *                segments (= connections' rx bytes) at once: frame
 *                discovery + FIN/opcode/mask/length extraction on the GPU.
 *   hvws_unmask  the per-byte XOR of websocket_parser_decode
 *                (http/websocket_parser.c:173-180) as called in place by
 *                WebSocketParser's on_frame_body (http/WebSocketParser.cpp:32-34),
 *                applied to every masked payload span the last scan found.
 *   hvws_step    scan + unmask: one pass of the hot path over a batch.
 *   hvws_rx_batch  the same from/to host memory (H2D, step, D2H).
 *   hvws_build_frames  transmit side: websocket_build_frame
 *                (http/websocket_parser.c:207-256, as called per message by
 *                WebSocketChannel::sendFrame via ws_build_frame,
 *                http/WebSocketChannel.cpp:66-79, http/wsdef.c:36-46)
 *                for a whole batch of outgoing frames at once.
 *   hvws_encode_keys  the handshake digest ws_encode_key (http/wsdef.c:11-20)
 *                for a batch of upgrade requests.
 *   hvws_utf8    RFC 6455 sec. 8.1 over the batch's text messages (the
 *                reference does not check it; opt-in).
 *   hvws_messages  WebSocketParser::FeedRecvData's message reassembly
 *                (http/WebSocketParser.cpp:8-75) for a whole batch: the
 *                payload bytes with the headers squeezed out, unmasked on the
 *                way, and the table of the messages they form -- on the device.
 *   hvws_messages_rfc  the same with RFC 6455's message rule in place of the
 *                reference's: control frames apart from the fragmented data
 *                message they interrupt, whole messages across batches.
 *   hvws_send_messages  WebSocketChannel::send (http/WebSocketChannel.cpp:5-48)
 *                for a batch of messages: one frame each, or fragmented into
 *                OPCODE, CONTINUE ..., CONTINUE + FIN, from a message table
 *                that may exist only on the device.
 *   hvws_replies  the server's onMessage dispatch (http/server/HttpHandler.cpp:
 *                174-200) over the pieces of hvws_messages: a PONG for every
 *                PING, a CLOSE for the first CLOSE and nothing after it,
 *                optionally an echo of data messages -- as a message table
 *                hvws_send_messages sends without a host read in between.
 *   hvws_fanout  TcpServerTmpl::broadcast / foreachChannel (evpp/TcpServer.h:
 *                182-199) per topic: the reply table expanded through a
 *                subscription table and ordered by destination connection.
 *   hvws_budget  hio_write's over-limit rule (event/nio.c:554-560) for that
 *                table: every destination's deliveries cut at its byte budget,
 *                the destinations that went over, each one's byte range.
 *   hvws_route   what a pub/sub server's onmessage does first (user code in the
 *                reference): each data message's command header read on the
 *                device -- publish to a topic, subscribe, unsubscribe -- into a
 *                topic per reply for hvws_fanout_routed and the join / leave
 *                events for hvws_subs_update.
 *   hvws_subs_update_routed  what the event loop does when a channel closes
 *                (evpp/TcpServer.h removeChannel) together with the turn's own
 *                subscribe commands: hvws_subs_update over the route's events, a
 *                drop per closed, failed, malformed or over-limit connection and
 *                the host's own events, merged on the device in that order.
 *   hvws_retain  a last-value cache (user code in the reference; MQTT's retained
 *                message): each topic's last publication kept in a
 *                device-resident store, and a snapshot row per subscribe of the
 *                turn for a second hvws_send_messages.
 *   hvws_envelope  what a broker puts in front of a delivery (STOMP's
 *                destination:, MQTT's topic name; user code in the reference):
 *                every reply's bytes written once into a second buffer,
 *                publications behind a line naming their topic and sender.
 *   hvws_sequence  what a broker's stream position is (MQTT's packet id, a
 *                log's offset; user code in the reference): every publication
 *                numbered within its topic from counters kept on the device.
 *   hvws_envelope_sequenced  hvws_envelope with that number on the line, so
 *                that a subscriber sees what hvws_budget cut and can order a
 *                retained snapshot against the live deliveries behind it.
 *   hvws_check  what the reference leaves out altogether: failing a connection
 *                that breaks the protocol (RFC 6455 sec. 7.1.7) -- the failing
 *                record and close code per connection, on the device; opt-in.
 *   hvws_wsp_*   C handle over the WebSocketParser class
 *                (http/WebSocketParser.h:19-31) for FFI callers.
 *
 * A batch is a buffer holding `nseg` segments; segment s is the byte range
 * [segs[s].off, segs[s].off + segs[s].len) and continues the stream whose
 * parser state is carry[s] (a `struct websocket_parser`).  Segments must be
 * sorted by offset and must not overlap.  Contexts are per (thread, device):
 * several event-loop threads may each own one; there is no global lock.
 * Device buffers passed in must be 16-byte aligned.
 */
#ifndef HVWS_H
#define HVWS_H

#include <stddef.h>
#include <stdint.h>

#include "websocket_parser.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    HVWS_OK = 0,
    HVWS_ENODEV = -1,   /* no HIP device / runtime */
    HVWS_EINVAL = -2,
    HVWS_ENOMEM = -3,
    HVWS_EHIP = -4      /* a HIP call failed; see hvws_last_error() */
};

/* hvws_frame.info bits */
#define HVWS_I_FLAGS       0xFFu      /* websocket_flags of the frame          */
#define HVWS_I_PHASE_SHIFT 8          /* 2-bit mask phase at pay_off           */
#define HVWS_I_HDR         (1u << 10) /* header completed here (on_frame_header fires) */
#define HVWS_I_BODY        (1u << 11) /* >= 1 payload byte here (on_frame_body fires)   */
#define HVWS_I_END         (1u << 12) /* frame completed here (on_frame_end fires)      */
#define HVWS_I_START       (1u << 13) /* first header byte is inside this segment       */
#define HVWS_I_INVALID     (1u << 14) /* header violates an enabled validation class    */
#define HVWS_I_VSHIFT      16         /* HVWS_V_* classes violated, bits 16-21           */

/* Optional protocol validation (hvws_set_validation), RFC 6455 sec. 5.1-5.5.
 * The reference checks none of these, so all are off by
 * default and results are then identical to the reference's. */
#define HVWS_V_RSV       (1u << 0)  /* RSV1-3 set (no extension is negotiated)        */
#define HVWS_V_OPCODE    (1u << 1)  /* reserved opcode 3-7 or 0xB-0xF                 */
#define HVWS_V_CONTROL   (1u << 2)  /* control frame with FIN = 0 or > 125 bytes      */
#define HVWS_V_LEN64     (1u << 3)  /* 64-bit length with its most significant bit set */
#define HVWS_V_NONMIN    (1u << 4)  /* length not in its minimal encoding             */
#define HVWS_V_UNMASKED  (1u << 5)  /* client-to-server frame without a mask          */
#define HVWS_V_ALL       0x3Fu

typedef struct hvws_ctx hvws_ctx;

typedef struct hvws_segment {
    uint64_t off;
    uint64_t len;
} hvws_segment;

/* One frame as seen by one batch (40 bytes). Offsets are absolute in the
 * batch buffer. */
typedef struct hvws_frame {
    int64_t  hdr_off;   /* first header byte, -1 if it was in an earlier batch */
    uint64_t pay_off;   /* first payload byte of this frame in the batch       */
    uint64_t pay_len;   /* payload bytes of this frame inside the batch        */
    uint64_t length;    /* full payload length (parser->length)                */
    uint32_t key;       /* masking key, mask[0] in bits 0-7 (0 if unmasked)    */
    uint32_t info;      /* HVWS_I_* */
} hvws_frame;

/* ---- context / memory ---------------------------------------------- */
int         hvws_device_count(void);
hvws_ctx*   hvws_ctx_create(int device);          /* NULL on failure */
void        hvws_ctx_destroy(hvws_ctx* ctx);
const char* hvws_last_error(void);                /* thread-local */
void*       hvws_ctx_stream(hvws_ctx* ctx);       /* hipStream_t */
int         hvws_ctx_device(hvws_ctx* ctx);
/* The PCI bus id ("dddd:bb:dd.f", NUL-terminated, len >= 13) of HIP device
 * `device` and, in *cur, the device hipGetDevice reports once it is selected:
 * a multi-GPU run names the physical card each rank used. */
int         hvws_device_identity(int device, char* bus_id, int len, int* cur);

void* hvws_dev_alloc(hvws_ctx* ctx, uint64_t bytes);
void  hvws_dev_free(hvws_ctx* ctx, void* p);
void* hvws_host_alloc(hvws_ctx* ctx, uint64_t bytes); /* pinned */
void  hvws_host_free(hvws_ctx* ctx, void* p);
int   hvws_h2d(hvws_ctx* ctx, void* dst, const void* src, uint64_t n);  /* async, ctx stream */
int   hvws_d2h(hvws_ctx* ctx, void* dst, const void* src, uint64_t n);  /* async, ctx stream */
int   hvws_memset(hvws_ctx* ctx, void* dst, int v, uint64_t n);
int   hvws_d2d(hvws_ctx* ctx, void* dst, const void* src, uint64_t n);  /* async, ctx stream */
int   hvws_sync(hvws_ctx* ctx);
/* Tests only: hold back work queued on the ctx stream after this call for
 * `usec` microseconds without occupying the device (a host function on the
 * stream), e.g. to keep an unmask waiting while the second stream runs on. */
int   hvws_debug_stall(hvws_ctx* ctx, uint32_t usec);

/* ---- the hot path, device resident ---------------------------------- */
/* Frame discovery + header parse for every segment.  Waits for the device
 * once (to size the frame table, or for its speculative table's check; see
 * hvws_set_speculation) -- not for earlier work on the stream to finish.
 * Results stay on the device in `ctx`. */
int hvws_scan(hvws_ctx* ctx, const uint8_t* d_rx, uint64_t rx_len, const hvws_segment* segs,
              const websocket_parser* carry_in, uint32_t nseg);
/* Unmask, in place, every masked payload span found by the last scan.
 * Asynchronous on the ctx stream. */
int hvws_unmask(hvws_ctx* ctx, uint8_t* d_rx, uint64_t rx_len);
/* scan + unmask */
int hvws_step(hvws_ctx* ctx, uint8_t* d_rx, uint64_t rx_len, const hvws_segment* segs,
              const websocket_parser* carry_in, uint32_t nseg);
/* hvws_step for a batch whose bytes are already complete in device memory
 * (nothing queued on the context stream still writes them).  Its discovery
 * then runs on the context's second stream, overlapping the unmask of the
 * previous step, whose tables are kept in the other of two table sets; the
 * unmask is queued on the context stream after it, as with hvws_step.  Frames
 * and carry of the call are readable (hvws_get_*) until the next scan; work
 * queued on the context stream afterwards sees the unmasked bytes.
 * A step that took the RUN path (hvws_set_run; hvws_step too) builds its
 * frames and carry when hvws_get_* / hvws_frame_count first asks, from the
 * batch's header bytes: those bytes must not change until then (reading them
 * before the next receive into the buffer, or calling hvws_frame_count right
 * after the step, fixes them).  Payload bytes may change freely. */
int hvws_step_resident(hvws_ctx* ctx, uint8_t* d_rx, uint64_t rx_len, const hvws_segment* segs,
                       const websocket_parser* carry_in, uint32_t nseg);

int64_t hvws_frame_count(hvws_ctx* ctx);
int     hvws_get_frames(hvws_ctx* ctx, hvws_frame* out, uint64_t first, uint64_t n);
/* first frame index and frame count of every segment of the last scan */
int     hvws_get_segment_frames(hvws_ctx* ctx, uint64_t* first, uint64_t* count);
/* parser state after each segment (WebSocketParser semantics: mask_offset
 * advanced over unmasked bytes).  started[s] = 1 when the pending frame's
 * first header byte lay inside segment s. */
int     hvws_get_carry(hvws_ctx* ctx, websocket_parser* out, int* started);

/* Device time (ms, HIP events on the ctx stream) of the last scan and
 * unmask: out[0] = scan kernels (count + offsets + emit + tile index),
 * out[1] = unmask kernel.  A pipelined step (hvws_step_resident) records the
 * unmask's events only: its out[0] is -1 ($HVWS_STEP_EVENTS=2 records both).
 * The small-batch path (reads of an event loop) records none unless
 * $HVWS_STEP_EVENTS=2: out[0] = out[1] = -1 (an event-carrying launch costs
 * ~10 us of a ~30 us read). */
int hvws_last_times(hvws_ctx* ctx, float out[2]);
/* The same for each of the last min(max_steps, 32) scans, oldest first:
 * out[2*i] = scan ms, out[2*i+1] = unmask ms (-1 if the step had none).
 * Waits for those steps only; returns the number of steps written (< 0 on
 * error).  Lets a caller time a run of asynchronous steps afterwards. */
int hvws_step_times(hvws_ctx* ctx, float* out, int max_steps);
/* Record those timing events on every `every`-th scan only (1, the default:
 * every scan; 0: none).  Each event-carrying step costs device time between
 * kernels -- ~15 us of a 0.38 ms pipelined config-2 step -- so a caller that
 * times a long run samples it (bench.py: every 8th step); unsampled steps
 * read -1.  Returns the previous interval (< 0 on error). */
int hvws_set_step_event_interval(hvws_ctx* ctx, uint32_t every);

/* k_unmask geometry.  By default it follows the batch size: 512 threads x 2
 * chunks in linear tile order below 16 GiB, 256 x 4 in XCD-contiguous order
 * from there (measured).  hvws_unmask_kernel_name: the name
 * of the forced geometry, or of the large-batch one; ..._for: the geometry a
 * batch of rx_len bytes runs with (e.g. "k_unmask<256,4,xcd>"). */
const char* hvws_unmask_kernel_name(void);
const char* hvws_unmask_kernel_name_for(uint64_t rx_len);
/* The RUN path's unmask kernel (HVWS_PATH_RUN steps), e.g. "k_unmask_run<256,4,lds>". */
const char* hvws_run_kernel_name(void);
/* Force a k_unmask geometry for later scans (tuning; process-wide); -1 =
 * back to the choice by batch size. */
int hvws_set_unmask_variant(int variant);

/* Uniform runs of at least `frames` predicted frames in one segment are
 * verified grid-wide (k_verify); shorter ones by the per-segment wave walk.
 * Tuning only (process-wide, default 4096, 0 = default); results never
 * depend on it.  Returns the previous value. */
uint64_t hvws_set_spec_min(uint64_t frames);

/* Frame sieve: one segment of at least `bytes` after its first whole frame,
 * whose frame sizes vary, is discovered by data-parallel passes (every byte
 * position tested for a plausible client frame header chained 3 headers
 * deep, then pointer doubling from the first frame along exact successors)
 * instead of the serial header-to-header walk; frames the chain cannot reach
 * (unmasked, RSV bits, reserved opcodes) are walked exactly from there.
 * Tuning only (process-wide, default 8 MiB, 0 = default; $HVWS_SIEVE_MIN);
 * results never depend on it.  Returns the previous value. */
uint64_t hvws_set_sieve_min(uint64_t bytes);

/* What the frame sieve did in the last one-segment scan on ctx (NULL = the
 * calling thread's context; waits for that scan): out[0] = 0 not run or not
 * wanted (uniform sizes, short segment), 1 sieved, 2 more survivors than its
 * table held (walked instead); out[1] = survivors; out[2] = frames on the
 * chain; out[3] = segment offset where the exact walk resumed. */
int hvws_last_sieve(hvws_ctx* ctx, uint64_t out[4]);

/* Frame-sieve windows.  A long stream of large frames is sieved only over the
 * first `window_bytes` of every region of about `hops` mean-sized frames (the
 * mean from the context's last exact count of a one-segment scan); the chain's
 * link walks cross the rest of each region frame by frame, so the sieve reads
 * window / region of the bytes instead of all of them.  hops = 0 sieves every
 * position (the round-2 behaviour).  Process-wide tuning (default 320 and
 * 1 MiB + 16 KiB; $HVWS_EXPERIMENT sieve_hops, sieve_window; window 0 = default);
 * results never depend on it.  prev (may be NULL) receives the old values. */
void hvws_set_sieve_windows(uint64_t hops, uint64_t window_bytes, uint64_t prev[2]);

/* Window geometry of the last sieved scan on ctx, in 8 KiB tiles: out[0] =
 * region, out[1] = window (equal: every tile sieved; 0, 0: no sieve ran). */
int hvws_last_sieve_windows(hvws_ctx* ctx, uint64_t out[2]);

/* Verify after every scan that frame ends (pay_off + pay_len) never
 * decrease over the table -- the invariant the unmask tile index is built on
 * -- and fail the scan with HVWS_EINVAL otherwise.  Costs one device sync
 * per scan; for tests (process-wide; default off, or $HVWS_CHECK_TABLES=1).
 * Returns the previous setting. */
int hvws_set_table_checks(int on);

/* Speculative frame tables for large multi-segment batches.  SPEC: when the
 * last batch's per-segment record counts matched the uniform-stride
 * estimates, the next scan emits straight into the table at the estimated
 * offsets and the device checks it (one walk, no host round trip before
 * EMIT).  SLACK: otherwise (mixed sizes), one walk emits each segment's
 * records into its own region of a scratch table (at most 1.5 x the last
 * exact scan's largest segment count + 16), the device checks that every
 * segment fit and compacts the records to the exact offsets (and whether the
 * uniform estimates would have held: SPEC next time).  A failed check
 * re-scans exactly (COUNT, wait, EMIT).  mode -1 = that automatic choice
 * (default, or $HVWS_EXPERIMENT spec unset), 0 = never speculate, 1 = try SPEC first,
 * 2 = try SLACK first (tests).  Results never depend on it.  ctx NULL = the
 * calling thread's context.  Returns the previous mode. */
int hvws_set_speculation(hvws_ctx* ctx, int mode);

/* One-walk passes (SPEC, SLACK): mode -1 = adaptive (default: the grid-wide
 * k_verify pair and k_head<true> run only when the last check saw a segment
 * with >= spec_min predicted frames; otherwise k_head<false>, the offsets and
 * one walk that also records the carried-in frame), 0 = never, 1 = always.
 * Results never depend on it.  Returns the previous mode. */
int hvws_set_walk_verify(hvws_ctx* ctx, int mode);

/* How the last hvws_scan on ctx found its frames (tests, benchmarks). */
enum {
    HVWS_PATH_COUNT_EMIT = 0,       /* COUNT then EMIT, table sized by the record bound, no wait */
    HVWS_PATH_COUNT_READ_EMIT = 1,  /* COUNT, wait for the count, EMIT */
    HVWS_PATH_SINGLE = 2,           /* one segment: one walk into an estimated table */
    HVWS_PATH_SPEC = 3,             /* speculative table checked exact on the device */
    HVWS_PATH_SPEC_FAILED = 4,      /* speculation rejected by the check, then COUNT/EMIT */
    HVWS_PATH_SLACK = 5,            /* mixed sizes: one EMIT walk into per-segment regions, compacted on the device */
    HVWS_PATH_SLACK_FAILED = 6,     /* a segment outgrew its region, then COUNT/EMIT */
    HVWS_PATH_RUN = 7               /* step of small uniform frames: per-segment run descriptors, headers
                                       checked by the unmask itself, records built when read */
};
int hvws_last_scan_path(hvws_ctx* ctx);

/* RUN path for hvws_step / hvws_step_resident: a batch of many segments whose
 * last exact scan found each segment one run of equal frames (and frames of at
 * most 8 KiB) is discovered by k_head alone -- the carried-in frame and the
 * frame cut by the segment end exactly, the run in between as a hypothesis --
 * and the unmask parses every run header from the bytes it loads anyway,
 * checks it against the hypothesis and takes its key from it: no per-frame
 * records and no second pass over the header lines.  A repair pass queued on
 * the context stream right behind undoes and redoes exactly any segment whose
 * hypothesis failed, so work queued after the step sees the reference's bytes
 * either way; the next steps then scan exactly until a check sees uniform
 * frames again.  The frame records, counts and carry of a RUN step are built
 * (an exact scan of the unchanged headers) when hvws_get_* first asks: the
 * header bytes must stay as they were until then (hvws_step_resident).  An
 * hvws_unmask after a RUN step builds them first and XORs by that exact
 * table.  mode
 * -1 = automatic (default; $HVWS_RUN=0 turns it off), 0 = never, 1 = every
 * step batch of several segments, whatever the last scan saw (tests).  ctx
 * NULL = the calling thread's context.  Returns the previous mode. */
int hvws_set_run(hvws_ctx* ctx, int mode);
/* Segments of the last step that the RUN path's repair pass put back and
 * unmasked exactly (their hypothesis failed, or k_head saw they were not one
 * run); -1 if the last scan was not a RUN step.  Waits for the step. */
int64_t hvws_last_run_repairs(hvws_ctx* ctx);

/* Device span of a timed region: hvws_span_begin records a marker on each of
 * the context's compute streams, hvws_span_end records the end markers, waits
 * for them and returns (latest end - earliest begin) in ms.  For benchmarks:
 * the per-device time of a run of steps. */
int hvws_span_begin(hvws_ctx* ctx);
int hvws_span_end(hvws_ctx* ctx, float* ms);
/* Batches whose record bound (rx_len / 2 + 2 * nseg + 1) is at most
 * `records` are scanned COUNT -> EMIT with the table sized by that bound
 * (default 2^24); larger ones wait for a count (or speculate).  1 makes
 * every multi-segment batch take the large-batch path, 0 restores the
 * default.  Tuning/testing only; results never depend on it.  Returns the
 * previous bound. */
uint64_t hvws_set_fast_bound(hvws_ctx* ctx, uint64_t records);

/* STREAM-style in-place ceiling: d[i] ^= pattern over n bytes (16-B aligned). */
int hvws_stream_xor(hvws_ctx* ctx, uint8_t* d, uint64_t n, uint32_t pattern);

/* ---- transmit side, device resident ---------------------------------- */
/* Build n frames back to back into d_out, each byte-identical to
 * websocket_build_frame(frame, flags[i], mask + i, payload + pay_off[i],
 * len[i]): header (FIN/opcode, MASK bit, 7/16/64-bit length, key) followed by
 * the payload XOR-masked from phase 0 when flags[i] has WS_HAS_MASK.
 * d_mask[i] holds frame i's key with mask[0] in bits 0-7; d_mask may be NULL
 * only if no frame is masked (the reference would read uninitialised bytes).
 * d_out_off (n words, optional) receives each frame's offset in d_out.
 * *out_len = total bytes.  Synchronises once (after sizing/validating the
 * tables: a payload range outside [0, payload_len) or an output larger than
 * out_cap is HVWS_EINVAL and nothing is written); the build kernel itself is
 * asynchronous on the ctx stream.  d_out must be 16-byte aligned and must not
 * overlap d_payload. */
int hvws_build_frames(hvws_ctx* ctx, uint8_t* d_out, uint64_t out_cap, const uint8_t* d_payload,
                      uint64_t payload_len, const uint64_t* d_pay_off, const uint64_t* d_len,
                      const uint8_t* d_flags, const uint32_t* d_mask, uint64_t n, uint64_t* d_out_off,
                      uint64_t* out_len);
/* Device time (ms, HIP events on the ctx stream) of the last hvws_encode_keys
 * kernel, or of the last hvws_build_frames' device work after its size check
 * (tile index, source spans, k_build), or of the last hvws_utf8 (its tile
 * index and all three kernels), or of the last hvws_messages (table pass,
 * tile index and gather), or of the last hvws_send_messages' device work after
 * its wait (expansion, tile index, spans, k_build), or of the last hvws_check
 * (its scan and table kernels), or of the last hvws_fanout's device work after
 * its wait (expansion, sort, finish), or of the last hvws_budget (all of it),
 * or of the last hvws_subs_update's after
 * its wait (the placement) -- whichever was called last; the default build
 * geometry's name. */
int hvws_last_kernel_ms(hvws_ctx* ctx, float* ms);
const char* hvws_build_kernel_name(void);
/* The k_build geometry the last hvws_build_frames on ctx ran: one-wave
 * workgroups of 4 KiB tiles, in a lean-LDS form for batches of small frames
 * (mean frame < 4 KiB), or $HVWS_EXPERIMENT build's.  Results never
 * depend on it. */
const char* hvws_last_build_kernel(hvws_ctx* ctx);
/* 1 when the last hvws_build_frames on ctx found a uniform layout (every frame
 * the same size and payload length, payload offsets a + k*b with b >= 0) and
 * built it without a tile index (each tile finds its frames from its
 * position); 0 otherwise.  Results never depend on it. */
int hvws_last_build_uniform(hvws_ctx* ctx);

/* ---- handshake, device resident --------------------------------------- */
/* Sec-WebSocket-Accept for n upgrade requests: accept + 32*i receives the 28
 * characters ws_encode_key (http/wsdef.c:11-20) writes for key i (the bytes
 * d_keys[key_off[i] .. + key_len[i]), no NUL inside), followed by 4 zero bytes
 * -- the callers' zeroed char[32] (http/server/HttpHandler.cpp:986).
 * d_accept must be 16-byte aligned.  Asynchronous on the ctx stream. */
int hvws_encode_keys(hvws_ctx* ctx, const char* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
                     uint64_t n, char* d_accept);

/* ---- host memory in, host memory out -------------------------------- */
/* Copies h_rx to the device, runs scan (+ unmask if `unmask`), copies the
 * bytes back in place and updates carry[].  Frames of the batch are then
 * available through hvws_get_frames(). */
int hvws_rx_batch(hvws_ctx* ctx, uint8_t* h_rx, uint64_t len, const hvws_segment* segs,
                  websocket_parser* carry, uint32_t nseg, int unmask);

/* Enable protocol validation classes (HVWS_V_*; 0 = off, the default) for
 * later batches on ctx (NULL = the calling thread's reference-API context).
 * Device API: a frame whose header violates an enabled class carries
 * HVWS_I_INVALID and the classes in its info.  Reference API: the library
 * rejects such a frame the way a failing on_frame_header callback would --
 * websocket_parser_execute / FeedRecvData return the index of the header's
 * last byte (< len), so HttpHandler::FeedRecvData reports ERR_PARSE and the
 * connection closes (http/server/HttpHandler.cpp:757-763); on_frame_header
 * is not called for it.  A header split across reads keeps its partial
 * validation state in the padding byte after websocket_parser.mask_offset.
 * A step under validation never takes the RUN path, even with
 * hvws_set_run(ctx, 1); the records of a RUN step read after a later
 * hvws_set_validation are those of the classes in force when it ran (none).
 * Returns the previous classes. */
uint32_t hvws_set_validation(hvws_ctx* ctx, uint32_t classes);

/* ---- UTF-8 validation of text messages, device resident ---------------- */
/* RFC 6455 sec. 5.6 / 8.1: a text message must be valid UTF-8 (RFC 3629).  The
 * reference does not check this; like hvws_set_validation it is new behaviour
 * a caller opts into, here by calling hvws_utf8 after a scan or step.
 *
 * The validator is a state machine over the payload bytes.  Its states say
 * what the next byte must be:
 *    0 HVWS_U8_ACCEPT  character boundary
 *    1                 one continuation 80..BF, then 0
 *    2                 80..BF, then 1
 *    3                 after E0: A0..BF, then 1
 *    4                 after ED: 80..9F, then 1
 *    5                 after F0: 90..BF, then 2
 *    6                 after F1..F3: 80..BF, then 2
 *    7                 after F4: 80..8F, then 2
 *   15 HVWS_U8_REJECT  sticky
 * and from state 0: 00..7F -> 0, C2..DF -> 1, E0 -> 3, E1..EC / EE / EF -> 2,
 * ED -> 4, F0 -> 5, F1..F3 -> 6, F4 -> 7, anything else -> 15.
 *
 * The transition word of a byte string holds, in nibble k (bits 4k..4k+3), the
 * state the string leaves the machine in when it is entered in state k
 * (k = 0..7).  The empty string gives HVWS_U8_IDENTITY; "abc" gives
 * 0xfffffff0; the bytes 82 AC give 0x11f0f0ff.  Words compose: a then b is
 * nibble-wise b[a[k]], and REJECT stays REJECT.  hvws_utf8 computes one word
 * per frame record of the last scan (the record's payload bytes inside the
 * batch; a record without payload bytes has the identity word), whatever the
 * frame's opcode, and then folds each segment's words in record order.
 *
 * The fold keeps one state word per segment (= per connection): bits 0-3 the
 * state above, bit 4 HVWS_U8_TEXT_OPEN (a text message is in progress); 0 is a
 * fresh connection.  For each record of the segment, in order, with
 * op = info & 0xF and fin = info & 0x10:
 *   - op >= 8 or op in 3..7: the record is skipped (control frames between the
 *     fragments of a message);
 *   - op == 1 with HVWS_I_HDR: text opens, state = ACCEPT (an unfinished
 *     earlier message is a protocol error of another kind: restart);
 *   - op == 2 with HVWS_I_HDR: text closes, state = ACCEPT;
 *   - op == 0, or a record without HVWS_I_HDR, keeps what is open (a lone
 *     continuation with nothing open is ignored);
 *   - text open and HVWS_I_BODY: state = word[state];
 *   - HVWS_I_END and fin with text open: a state other than ACCEPT becomes
 *     REJECT (a character truncated by the end of the message); text closes.
 * bad[s] is the index (in the batch's frame table) of the first record at
 * which the state became REJECT, or HVWS_U8_NONE.  REJECT is sticky: later
 * records change neither the state word nor bad[s], and the state word is then
 * HVWS_U8_REJECT alone (bit 4 clear), so the result does not depend on where
 * the batches cut the stream.  A state word carried in with REJECT (or with
 * 8..14, which are no states) gives bad[s] = the segment's first record index
 * (even when the segment has no records) and carries out REJECT.  A Close
 * frame's reason text is not checked (hvws_check's HVWS_C_CLOSE_UTF8 does).
 *
 * An event loop keeps one uint32_t per connection next to its
 * websocket_parser carry: 0 at accept, state_in[s] on the way in, state_out[s]
 * on the way out, and fails the connection (close code 1007) when bad[s] is
 * not HVWS_U8_NONE. */
#define HVWS_U8_ACCEPT    0u
#define HVWS_U8_REJECT    15u
#define HVWS_U8_TEXT_OPEN (1u << 4)
#define HVWS_U8_IDENTITY  0x76543210u
#define HVWS_U8_NONE      UINT64_MAX
/* After hvws_scan / hvws_step[_resident] of d_rx (same buffer and length as the last
 * scan, else HVWS_EINVAL; none before it: HVWS_EINVAL). masked: 1 = masked payloads
 * are still masked (after hvws_scan), 0 = already unmasked (after a step).
 * state_in: host, nseg words, NULL = all 0. Asynchronous on the ctx stream.
 * The buffer is only read.  After a RUN step the frame records are built first
 * (as for hvws_get_frames). */
int hvws_utf8(hvws_ctx* ctx, const uint8_t* d_rx, uint64_t rx_len, int masked, const uint32_t* state_in);
/* Results of the last hvws_utf8 on ctx, valid until the next one.  Both wait
 * for it.  hvws_get_utf8_words: the words of records first .. first + n - 1
 * (HVWS_EINVAL beyond that batch's record count).  hvws_get_utf8: per segment
 * of that batch, the state word to carry into the connection's next batch and
 * bad[s] (either may be NULL). */
int hvws_get_utf8_words(hvws_ctx* ctx, uint32_t* out, uint64_t first, uint64_t n);
int hvws_get_utf8(hvws_ctx* ctx, uint32_t* state_out, uint64_t* bad);
/* Records of the batch the last hvws_utf8 ran over (-1: none yet); waits.  The
 * words outlive the next scans, hvws_frame_count does not. */
int64_t hvws_utf8_count(hvws_ctx* ctx);
/* Bytes of the batch one workgroup of the word kernel covers (tests place
 * payload bytes around its multiples). */
uint64_t hvws_utf8_tile(void);

/* ---- message reassembly, device resident -------------------------------- */
/* What WebSocketParser::FeedRecvData (http/WebSocketParser.cpp:8-75) delivers
 * through onMessage, for every segment of a batch, without the bytes leaving
 * the device.  Per connection the reference keeps a latched opcode and a
 * growing message; over the frame records of a segment, in frame-table order,
 * its rule (quirks of SURVEY.md Appendix A included) is:
 *   - a record with HVWS_I_HDR whose opcode (info & 0xF) is non-zero latches
 *     that opcode; a CONTINUE keeps the latch; a connection that has latched
 *     nothing reports 8 (WS_OP_CLOSE, the constructor's value, Q6);
 *   - the payload bytes of EVERY record are appended, whatever the opcode: a
 *     control frame between two fragments lands in the message (Q5: text "AB"
 *     not final, ping "PING", final continuation "CD" deliver (9, "ABPING") and
 *     (9, "CD")); zero-length frames append nothing (Q7);
 *   - a record with HVWS_I_END and FIN (info & 0x10) completes the message:
 *     onMessage(latched opcode, bytes since the previous completion) fires and
 *     the next record starts a new message.
 *
 * Output.  d_out receives the payload bytes of the batch with the headers
 * squeezed out: record r's pay_len[r] bytes start at out_off[r] = the sum of
 * pay_len[q] over q < r, so segments are in order and each segment's bytes
 * are contiguous.  The message table holds pieces: a piece is the part of one
 * message that lies in this batch.  Each FIN-ended record closes a piece; the
 * records of a segment after its last FIN-ended one (all of its records when
 * it has none) form one trailing open piece, possibly of 0 bytes.  Pieces are
 * ordered by segment, then stream order; the table is dense.
 *
 * State.  An event loop keeps one hvws_msg_state per connection beside its
 * websocket_parser carry: all zero at accept, state_in[s] on the way in,
 * hvws_get_msg_state's on the way out.
 *   - opcode out is the latch after the segment's last record;
 *   - a segment with a FIN-ended record: open = 1 when records follow the last
 *     such record, else 0; pending = the trailing piece's len (0 without one);
 *   - a segment without one: open = state_in.open || it has records,
 *     pending = state_in.pending + the segment's bytes;
 *   - a segment without records returns its state unchanged and has no pieces;
 *   - a state_in with open == 0 and pending != 0, or with opcode > 15, is
 *     HVWS_EINVAL.
 * Concatenating a message's pieces across batches is the caller's: the piece
 * with HVWS_M_END gives the message's length in `total`.  (hvws_messages_joined,
 * below, does it on the device.) */
typedef struct hvws_msg_state {   /* 16 B per connection; all zero = fresh */
    uint64_t pending;             /* bytes of the open message delivered in earlier batches' pieces */
    uint32_t opcode;              /* latched opcode, 0 = none latched yet */
    uint32_t open;                /* 1 = a message is open (pieces without HVWS_M_END precede) */
} hvws_msg_state;
typedef struct hvws_msg {         /* 40 B */
    uint64_t off, len;            /* the piece in d_out */
    uint64_t total;               /* message bytes so far: pending carried in (first piece of the segment only) + len */
    uint64_t rec;                 /* frame-table index of the piece's last record (joins hvws_utf8's bad[s]) */
    uint32_t seg;
    uint32_t info;                /* bits 0-3: opcode onMessage reports at that record; HVWS_M_END; HVWS_M_CONT */
} hvws_msg;
#define HVWS_M_END  (1u << 4)     /* a FIN frame ended here: the message is complete */
#define HVWS_M_CONT (1u << 5)     /* first piece of a segment whose state_in.open was set */
/* After hvws_scan / hvws_step[_resident] of d_rx (same buffer and length as
 * the last scan, else HVWS_EINVAL; none before it: HVWS_EINVAL).  masked: 1 =
 * payloads are still masked (after hvws_scan) and are XORed on the fly at each
 * record's key and phase, records without a mask copied as they are -- the
 * batch is never unmasked in place, receive-to-messages costs one read and one
 * write of the payload; 0 = already unmasked (after a step).  d_rx is only
 * read.  After a RUN step the frame records are built first (as for
 * hvws_get_frames).  state_in: host, nseg entries, NULL = all fresh.
 * Asynchronous on the ctx stream.  d_out must be 16-byte aligned and must not
 * overlap [d_rx, d_rx + rx_len), else HVWS_EINVAL.  With out_cap >= rx_len the
 * call does not wait (the payload cannot exceed the batch); with a smaller
 * out_cap it waits once for the payload total and returns HVWS_EINVAL, nothing
 * written, if that does not fit.  No byte of d_out at or beyond the payload
 * total is ever written.  hvws_last_kernel_ms reports this pass when it was
 * the last one called (the wait of a small out_cap included).  Results never
 * depend on the scan path. */
int hvws_messages(hvws_ctx* ctx, const uint8_t* d_rx, uint64_t rx_len, int masked, uint8_t* d_out, uint64_t out_cap,
                  const hvws_msg_state* state_in);
/* Results of the last hvws_messages on ctx, valid until the next one; all but
 * hvws_messages_device wait for it.  hvws_msg_count: its pieces (-1: none
 * yet).  hvws_msg_bytes: the bytes it wrote to d_out.  hvws_get_messages:
 * pieces first .. first + n - 1 (HVWS_EINVAL beyond the count).
 * hvws_get_segment_messages: per segment its first piece and piece count
 * (either may be NULL).  hvws_get_msg_state: per segment, the state to carry
 * into the connection's next batch.  hvws_messages_device: the piece table in
 * device memory, for a consumer kernel queued on the ctx stream (NULL: none
 * yet); it reads hvws_msg_count entries, a number such a kernel takes from the
 * host or bounds by the batch's record count. */
int64_t hvws_msg_count(hvws_ctx* ctx);
int hvws_msg_bytes(hvws_ctx* ctx, uint64_t* total);
int hvws_get_messages(hvws_ctx* ctx, hvws_msg* out, uint64_t first, uint64_t n);
int hvws_get_segment_messages(hvws_ctx* ctx, uint64_t* first, uint64_t* count);
int hvws_get_msg_state(hvws_ctx* ctx, hvws_msg_state* out);
const hvws_msg* hvws_messages_device(hvws_ctx* ctx);
/* Output bytes one workgroup of the gather covers at most: it runs in one of
 * two geometries, by the batch's mean bytes per record or $HVWS_EXPERIMENT
 * msg = 0 / 1, and the smaller tile divides this one
 * (tests place record boundaries around its multiples).  Results never depend
 * on the geometry. */
uint64_t hvws_msg_tile(void);

/* ---- whole messages across batches ---------------------------------------- */
/* hvws_messages with the bytes of every connection's open message kept on the
 * device between batches, so that every piece with HVWS_M_END is the complete
 * message, contiguous in d_out, and hvws_replies / hvws_send_messages answer
 * it with no host copy (no segment is HVWS_RF_DEFERRED).  The library keeps no
 * per-connection memory: the previous call's output is the pending store.  The
 * caller alternates two (or more) output buffers; the trailing open piece a
 * batch leaves for a connection is a byte range of that batch's d_out, and the
 * next batch copies that range (already unmasked, copied as it is) to the front
 * of the connection's part of the new d_out and appends the new payload bytes.
 * A connection with an open message and no read in a batch is passed as a
 * segment of length 0 -- its bytes are carried forward -- or, by a caller that
 * keeps older output buffers alive, left out of the batch.
 *
 * Everything hvws_messages documents holds (the preconditions on the scan,
 * d_rx and masked, the records of a RUN step, asynchrony, hvws_last_kernel_ms,
 * all getters, hvws_replies afterwards) except, with P[s] = state_in[s].pending
 * (0 when state_in is NULL):
 *   Carried bytes.  prev_off: host, nseg words; segment s's carried bytes are
 *     d_prev[prev_off[s] .. prev_off[s] + P[s]); prev_off[s] is ignored when
 *     P[s] == 0.  d_prev and prev_off may be NULL only when every P[s] is 0.
 *     d_prev must be 16-byte aligned; ranges may start at any byte and may
 *     overlap each other.  HVWS_EINVAL, nothing written: a pending byte without
 *     d_prev or prev_off; a range outside [0, prev_len); d_out[0, out_cap)
 *     overlapping d_rx[0, rx_len) or d_prev[0, prev_len).  No read leaves
 *     [d_prev, d_prev + prev_len) or the batch.
 *   Output.  Segments are in order; segment s's part of d_out is its P[s]
 *     carried bytes, then its records' payload bytes as hvws_messages lays
 *     them out; record r's bytes start at the sum of all carried and payload
 *     bytes before it.  hvws_msg_bytes is the sum of P[s] plus the payload
 *     bytes; no byte of d_out at or beyond that total is written.
 *   Pieces.  The rule is unchanged, but the first piece of a segment with
 *     P[s] > 0 starts at the segment's carried bytes and its len includes
 *     them: total == len for every piece.  HVWS_M_CONT, the opcode, rec and
 *     seg are as in hvws_messages.  A segment without records and with
 *     P[s] > 0 has exactly one piece: open, len = total = P[s], rec =
 *     HVWS_MSG_NOREC, opcode bits state_in[s].opcode (8 when that is 0),
 *     HVWS_M_CONT set; with P[s] == 0 it has none.  The table may hold up to
 *     nseg pieces more than the batch has records.  state_out equals what
 *     hvws_messages returns for the same inputs.
 *   out_cap.  No wait when out_cap >= rx_len + the sum of P[s] (saturating);
 *     otherwise one wait for the total, and HVWS_EINVAL with nothing written if
 *     it does not fit.
 * With every P[s] == 0 the bytes, tables, states and counts equal
 * hvws_messages' exactly.  hvws_replies after it runs unchanged; the
 * HVWS_MSG_NOREC piece has no HVWS_M_END, so it selects and indexes nothing.
 *
 * Cost: a message of L bytes delivered over k batches is copied about k*L/2
 * bytes in total.
 *
 * hvws_get_msg_carry (waits): off[s] = the offset in this call's d_out of
 * segment s's trailing open piece -- the connection's prev_off in its next
 * batch -- and 0 when state_out[s].pending == 0.  HVWS_EINVAL after a plain
 * hvws_messages. */
#define HVWS_MSG_NOREC UINT64_MAX
int hvws_messages_joined(hvws_ctx* ctx, const uint8_t* d_rx, uint64_t rx_len, int masked, uint8_t* d_out,
                         uint64_t out_cap, const hvws_msg_state* state_in, const uint8_t* d_prev, uint64_t prev_len,
                         const uint64_t* prev_off);
int hvws_get_msg_carry(hvws_ctx* ctx, uint64_t* off);

/* ---- RFC 6455 messages: control frames apart from fragmented messages ------ */
/* hvws_messages_joined with the message rule of RFC 6455 sec. 5.4 in place of
 * the reference's (quirk Q5 above): a control frame between the fragments of a
 * data message is a message of its own and does not land in the data message.
 * Text "AB" (not final), ping "PING", final continuation "CD" deliver
 * (1, "ABCD") and (9, "PING").  For a server of its own on the batch interface;
 * the drop-in, hvws_messages and hvws_messages_joined keep libhv's behaviour.
 *
 * The rule is the joined form's, applied to TWO VIRTUAL CONNECTIONS per
 * connection.  Over segment s's frame records in frame-table order, with op =
 * info & 0xF:
 *   - data records: op < 8 and at least one of HVWS_I_HDR, HVWS_I_BODY,
 *     HVWS_I_END set; they form virtual connection 2s;
 *   - control records: op >= 8 with the same condition; they form 2s + 1;
 *   - a record with none of the three bits (its header is still incomplete, it
 *     has no payload bytes) belongs to neither.
 * Each virtual connection follows hvws_messages_joined's contract exactly --
 * its own carried span, latch, pieces, trailing open piece and HVWS_MSG_NOREC
 * piece -- with two differences:
 *   1. in the control class every record with HVWS_I_END closes a piece, with
 *      or without FIN: a control frame is a message of its own;
 *   2. a data piece with nothing latched reports opcode 0, not 8 (Q6 is not
 *      reproduced: a lone final CONTINUE on a fresh connection selects no
 *      reply).
 * A new data header with a non-zero opcode while a data message is open
 * overwrites the latch and appends, as in the other forms; failing such
 * sequences, and every other protocol error, is not this call's (hvws_check,
 * below, does it).
 *
 * Output.  Connections are in order; connection s's part of d_out is its
 * carried data bytes, the payload of its data records in stream order, its
 * carried control bytes, the payload of its control records in stream order.
 * Every HVWS_M_END piece is a whole message, contiguous in d_out, total ==
 * len.  Pieces are ordered by connection, data pieces before control pieces;
 * seg is the connection; rec is the frame-table index of the piece's last
 * record and gives the stream order between the two classes (HVWS_MSG_NOREC
 * for a piece of carried bytes only); HVWS_M_CTL marks control pieces.
 * hvws_get_segment_messages gives each connection one first and one count over
 * both classes.  The table may hold up to 2 * nseg pieces more than the batch
 * has records.
 *
 * State.  One hvws_rfc_state per connection, in and out, all zero at accept.
 * On the way in data_off / ctl_off point into d_prev and are ignored when the
 * class's pending is 0; hvws_get_rfc_state (waits) returns the state on the
 * way out, its offsets pointing into this call's d_out (0 when nothing is
 * pending).  hvws_get_msg_state and hvws_get_msg_carry are HVWS_EINVAL after
 * this call, hvws_get_rfc_state after the other two forms.
 *
 * The joined form's preconditions hold, each for both classes: HVWS_EINVAL
 * with nothing written for a state no getter returns, a pending byte without
 * d_prev, a carried range outside [0, prev_len), a misaligned d_out or d_prev,
 * d_out overlapping the batch or d_prev; no read leaves the batch or d_prev; no
 * byte at or beyond hvws_msg_bytes (all carried and payload bytes) is written;
 * the records of a RUN step are built first; asynchronous on the ctx stream,
 * reported by hvws_last_kernel_ms.  No wait when out_cap >= rx_len + all
 * pending bytes of both classes (saturating); otherwise one wait, and
 * HVWS_EINVAL with nothing written if the total does not fit.
 *
 * hvws_replies after this call: selection by opcode and policy is unchanged,
 * but "close is final" goes by stream order.  With c the connection's selected
 * CLOSE piece of the smallest rec, a piece produces a reply only if its rec <=
 * rec(c), and of two pieces with that rec only c itself: a data message
 * completing after the CLOSE frame is not echoed, a PING after it is not
 * answered, a PING before it is.  Replies stay dense and in piece order, each
 * connection's data replies before its control replies, so its CLOSE reply is
 * the last frame of its byte range in the send's output.  HVWS_RF_DEFERRED is
 * never set; closed_in works as for the other forms.   */
typedef struct hvws_rfc_state {   /* 48 B per connection; all zero = fresh */
    hvws_msg_state data, ctl;     /* the data class's and the control class's state */
    uint64_t data_off, ctl_off;   /* where each class's pending bytes begin: in d_prev (in), in d_out (out) */
} hvws_rfc_state;
#define HVWS_M_CTL (1u << 6)      /* a piece of the control class (hvws_messages_rfc only) */
int hvws_messages_rfc(hvws_ctx* ctx, const uint8_t* d_rx, uint64_t rx_len, int masked, uint8_t* d_out,
                      uint64_t out_cap, const hvws_rfc_state* state_in, const uint8_t* d_prev, uint64_t prev_len);
int hvws_get_rfc_state(hvws_ctx* ctx, hvws_rfc_state* out);

/* ---- batched send, device resident ---------------------------------------- */
/* WebSocketChannel::send (http/WebSocketChannel.cpp:5-48) for n messages at
 * once.  Message i is the bytes [off, off + len) of d_payload and goes out
 * exactly as the reference's send(buf, len, fragment, opcode) builds it, with
 * F = fragment (0 = 65535, the reference's default) and L = len:
 *   - L <= F (L = 0 included): one frame with the message's opcode, its FIN bit
 *     taken from flags (send()'s `fin`);
 *   - otherwise ceil(L / F) frames: the first with the opcode and FIN clear,
 *     then CONTINUE frames of F bytes, then a last CONTINUE frame of
 *     L - (frames - 1) * F bytes (1 .. F) with FIN set.
 * Two reference quirks are reproduced: a fragmented message always ends with
 * FIN (the 4-argument send drops its `fin` argument when it fragments), and
 * control opcodes are fragmented like any other (send(msg, WS_OPCODE_PONG) with
 * a long message does that).
 *
 * Each frame is byte-identical to websocket_build_frame for its flags, length
 * and key.  masked == 0: server frames, no key; masked == 1: every frame has
 * WS_HAS_MASK, and where the reference draws rand() per frame, fragment j of a
 * message with key k uses hvws_frag_key(k, j).  Frames lie back to back in
 * d_out, messages in table order; messages may overlap or coincide in
 * d_payload (a broadcast).
 *
 * d_n (optional): a device word holding the message count; the effective count
 * is min(*d_n, n), read on the device (hvws_reply_count_device: the reply table
 * is sent without a wait in between).  d_msg_off (optional): effective count
 * + 1 words, the output offset of each message's first frame and the total in
 * the last.  *out_len receives the total bytes, *out_frames the frame count.
 *
 * Waits once, as hvws_build_frames does: after the message pass the host reads
 * {frames, bytes, bad messages}.  A message outside [0, payload_len), a flag
 * bit outside 0x1F, more than 2^32 - 2 frames, or a total above out_cap
 * (*out_len is still set then) is HVWS_EINVAL with nothing written to d_out; a
 * bad message adds nothing to the sums, and the sums saturate instead of
 * wrapping.  Everything after the wait is asynchronous on the ctx stream.
 * d_out must be 16-byte aligned and must not overlap d_payload.
 * hvws_last_kernel_ms reports the device work after the wait (expansion into
 * frames, tile index, spans, build) when this was the last call;
 * hvws_last_build_kernel / hvws_last_build_uniform report its k_build.
 * Results never depend on the geometry or on whether a uniform layout (every
 * message one frame of one length, payloads at a constant step) was found. */
typedef struct hvws_tx_msg {   /* 24 B */
    uint64_t off, len;         /* the message's bytes in d_payload */
    uint32_t flags;            /* bits 0-3 opcode, WS_FIN (0x10) = send()'s `fin`; any other bit: HVWS_EINVAL */
    uint32_t key;              /* masking key of the message, mask[0] in bits 0-7; used only when masked */
} hvws_tx_msg;
/* The key of fragment j of a message with key k (j = 0: k itself). */
static inline uint32_t hvws_frag_key(uint32_t k, uint32_t j) {
    uint32_t x = k + j * 0x9E3779B9u;
    if (j == 0) return k;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
int hvws_send_messages(hvws_ctx* ctx, uint8_t* d_out, uint64_t out_cap, const uint8_t* d_payload, uint64_t payload_len,
                       const hvws_tx_msg* d_msgs, uint64_t n, const uint64_t* d_n, uint64_t fragment, int masked,
                       uint64_t* d_msg_off, uint64_t* out_len, uint64_t* out_frames);

/* ---- server replies, device resident ------------------------------------- */
/* What the server's onMessage does with each message of the last
 * hvws_messages (http/server/HttpHandler.cpp:174-200), as a table of messages
 * to send.  Over that call's pieces in table order; only pieces with
 * HVWS_M_END count, and op is the piece's opcode (info & 0xF: what onMessage
 * reports, quirks Q5 and Q6 of SURVEY.md Appendix A included):
 *   - op 9 with HVWS_R_PONG in the policy: a reply with opcode 10;
 *   - op 8 with HVWS_R_CLOSE: a reply with opcode 8;
 *   - op 1 or 2 with HVWS_R_ECHO: a reply with the same opcode;
 *   - anything else: none.
 * Every reply has FIN set and carries the piece's bytes: off / len index the
 * d_out of that hvws_messages.
 * Close is final: after a segment's first piece selected as a CLOSE no later
 * piece of the segment produces a reply (Channel::close() sets CLOSED and
 * write() then fails, evpp/Channel.h:154-156,189-197); a segment with
 * closed_in[s] set produces none at all.  Both leave HVWS_RF_CLOSED in the
 * segment's flags: the caller carries it beside its other per-connection
 * state and closes the socket.
 * Deferred: a selected piece whose total != len completes a message begun in
 * an earlier batch; its bytes are not all in this d_out, so it produces no
 * reply here and its segment gets HVWS_RF_DEFERRED.  Only a segment's first
 * piece can be in this position: the host builds that one reply from its own
 * copy and sends it before the segment's device replies.  A deferred CLOSE
 * still closes the segment for the pieces after it.
 * Replies are dense, ordered by segment and then stream order, so each
 * segment's reply frames are contiguous in the send's output: from
 * d_msg_off[first[s]] to d_msg_off[first[s] + count[s]].
 *
 * hvws_replies runs after hvws_messages (none before it: HVWS_EINVAL), is
 * asynchronous on the ctx stream and does not wait.  closed_in: host, nseg
 * bytes, NULL = none.  Its results are valid until the next hvws_replies or
 * hvws_messages on ctx.  hvws_replies_device / hvws_reply_count_device: the
 * table and its count in device memory (d_msgs and d_n of
 * hvws_send_messages); hvws_reply_capacity: the entries the table holds (its
 * n).  hvws_reply_count, hvws_get_replies (replies first .. first + n - 1 and
 * the piece each answers; either may be NULL), hvws_get_segment_replies (per
 * segment, its first reply and reply count) and hvws_get_reply_flags (per
 * segment, HVWS_RF_*) wait. */
#define HVWS_R_PONG   1u  /* PING  -> PONG with the ping's message        (HttpHandler.cpp:181-185) */
#define HVWS_R_CLOSE  2u  /* CLOSE -> CLOSE with the same message; the
                             connection sends nothing after it             (HttpHandler.cpp:177-180) */
#define HVWS_R_ECHO   4u  /* TEXT / BINARY -> same opcode and bytes (an echo service's onmessage) */
#define HVWS_R_SERVER (HVWS_R_PONG | HVWS_R_CLOSE)
#define HVWS_RF_CLOSED   1u
#define HVWS_RF_DEFERRED 2u
int hvws_replies(hvws_ctx* ctx, uint32_t policy, const uint8_t* closed_in);
const hvws_tx_msg* hvws_replies_device(hvws_ctx* ctx);
const uint64_t* hvws_reply_count_device(hvws_ctx* ctx);
uint64_t hvws_reply_capacity(hvws_ctx* ctx);
int64_t hvws_reply_count(hvws_ctx* ctx);
int hvws_get_replies(hvws_ctx* ctx, hvws_tx_msg* out, uint64_t* piece, uint64_t first, uint64_t n);
int hvws_get_segment_replies(hvws_ctx* ctx, uint64_t* first, uint64_t* count);
int hvws_get_reply_flags(hvws_ctx* ctx, uint8_t* out);

/* ---- failing a connection, device resident (RFC 6455 sec. 7.1.7) ---------- */
/* Which connections of a batch broke the protocol, at which record and with
 * which close code -- joined on the device from the tables the earlier passes
 * left there, so a server on the batch interface need not read the frame
 * table, the piece table and the UTF-8 verdicts back and walk them per
 * connection before it may send.  The reference fails nothing; like
 * hvws_set_validation and hvws_utf8 this is behaviour a caller opts into.
 *
 * hvws_check runs after hvws_messages_rfc on ctx: HVWS_EINVAL after no message
 * call, after hvws_messages or hvws_messages_joined, or when a scan has run on
 * ctx since that hvws_messages_rfc.  It is asynchronous on the ctx stream, does
 * not wait and writes nothing another pass reads; hvws_last_kernel_ms reports
 * it when it was the last call.  The message call's d_out must still hold that
 * call's bytes: the pass reads the Close bodies there.
 *
 * State.  One uint32_t per connection beside its hvws_rfc_state: 0 at accept,
 * state_in[s] on the way in (host, nseg words, NULL = all 0), hvws_get_check's
 * state_out[s] on the way out.  HVWS_CK_OPEN: a data message is open;
 * HVWS_CK_FAILED: the connection has failed (sticky).  Any other bit in
 * state_in is HVWS_EINVAL.  A word carried in with HVWS_CK_FAILED gives
 * fail_rec[s] = the connection's first record index (even when it has no
 * records, as hvws_utf8 does it), why[s] = 0 and code[s] = 0 -- the batch that
 * failed it reported them -- and carries out HVWS_CK_FAILED alone.
 *
 * Classes (bits of `classes`; any other bit: HVWS_EINVAL), where each finds
 * its violation, and the close code it stands for:
 *   HVWS_C_HEADER      a record with HVWS_I_INVALID (the hvws_set_validation
 *                      classes in force when it was scanned): that record, 1002;
 *   HVWS_C_SEQUENCE    sec. 5.4: a record with HVWS_I_HDR and opcode 0 while no
 *                      data message is open, or opcode 1 / 2 while one is: that
 *                      record, 1002;
 *   HVWS_C_CLOSE_BODY  sec. 5.5.1, 7.4: a complete control piece of opcode 8
 *                      (HVWS_M_END and HVWS_M_CTL) whose len is 1 or above 125,
 *                      or whose big-endian code (its first two bytes) is outside
 *                      1000-1003, 1007-1011 and 3000-4999: the piece's rec, 1002;
 *   HVWS_C_CLOSE_UTF8  such a piece of 3 .. 125 bytes whose bytes from the third
 *                      on are not UTF-8 by hvws_utf8's machine (entered in
 *                      ACCEPT, ACCEPT at the end): the piece's rec, 1007;
 *   HVWS_C_TEXT_UTF8   the bad[s] of the last hvws_utf8 on ctx: that record,
 *                      1007.  That hvws_utf8 must have run over the scan the
 *                      message call ran over (no scan between them, the same
 *                      segments), else HVWS_EINVAL;
 *   HVWS_C_SIZE        with max_message > 0: a data record (opcode < 8) with
 *                      HVWS_I_HDR whose `length` exceeds max_message: that
 *                      record; or a data piece, open or complete, whose len
 *                      exceeds it: the piece's rec; 1009.  The check by piece is
 *                      batch-granular: a message that grows past the limit over
 *                      several frames is failed at the last record its piece has
 *                      in the batch in which it crossed, not at the frame that
 *                      crossed.
 * A piece whose rec is HVWS_MSG_NOREC takes the connection's first record
 * index.  A Close piece of more than 125 bytes is judged from its len and never
 * read; no read of a Close body leaves [off, off + len) rounded outwards to 16
 * bytes and clipped to [0, out_cap) of the message call.
 *
 * The sequence rule walks connection s's records in frame-table order from
 * HVWS_CK_OPEN of state_in[s].  Only records with HVWS_I_HDR and opcode 0, 1 or
 * 2 matter: such a record is checked against the open bit and then SETS it to
 * "FIN clear", whether or not it violated.  Opcodes 3-7 (the header class's)
 * and control records leave it alone.  state_out's HVWS_CK_OPEN is the bit
 * after the connection's last record.
 *
 * Verdict.  fail_rec[s] is the smallest record index at which an enabled class
 * found a violation, HVWS_CHECK_NONE without one; why[s] the HVWS_C_* bits of
 * all violations found at exactly that record; code[s] the close code of
 * why[s]'s lowest set bit, 0 when nothing failed; state_out[s] is
 * HVWS_CK_FAILED alone when fail_rec[s] is set.  What lies at or after the
 * failing record does not change the verdict.
 *
 * hvws_get_check (waits; any pointer may be NULL) returns the four per
 * connection of the last hvws_check; hvws_check_device is fail_rec[] in device
 * memory (NULL: none yet), valid until the next hvws_check.
 *
 * hvws_replies_checked is hvws_replies after hvws_messages_rfc with one more
 * rule: a piece whose rec >= fail_rec[s] of the last hvws_check produces no
 * reply -- a CLOSE piece exactly at that record included: a Close that is itself
 * malformed is not echoed.  Pieces before the failure reply as in hvws_replies,
 * and an earlier CLOSE stays final.  A failed connection gets HVWS_RF_FAILED |
 * HVWS_RF_CLOSED in its flags: the host appends the 4-byte frame 88 02 <code,
 * big-endian> behind that connection's reply range (d_msg_off[first[s] +
 * count[s]]) and closes the socket -- failures are rare and the host acts on the
 * socket anyway.  HVWS_EINVAL unless hvws_check ran on the last message call.
 * hvws_replies itself is unchanged.   */
#define HVWS_C_HEADER     (1u << 0)
#define HVWS_C_SEQUENCE   (1u << 1)
#define HVWS_C_CLOSE_BODY (1u << 2)
#define HVWS_C_CLOSE_UTF8 (1u << 3)
#define HVWS_C_TEXT_UTF8  (1u << 4)
#define HVWS_C_SIZE       (1u << 5)
#define HVWS_C_ALL        0x3Fu
#define HVWS_CK_OPEN      1u
#define HVWS_CK_FAILED    2u
#define HVWS_CHECK_NONE   UINT64_MAX
#define HVWS_RF_FAILED    4u
int hvws_check(hvws_ctx* ctx, uint32_t classes, uint64_t max_message, const uint32_t* state_in);
int hvws_get_check(hvws_ctx* ctx, uint32_t* state_out, uint64_t* fail_rec, uint32_t* why, uint16_t* code);
const uint64_t* hvws_check_device(hvws_ctx* ctx);   /* fail_rec[] in device memory */
int hvws_replies_checked(hvws_ctx* ctx, uint32_t policy, const uint8_t* closed_in);

/* ---- fan-out to topic subscribers, device resident ------------------------ */
/* hvws_replies answers the sender.  hvws_fanout delivers: it expands the reply
 * table of the last hvws_replies / hvws_replies_checked through a subscription
 * table and orders the result by destination connection, so that one
 * hvws_send_messages builds the turn's whole output with every destination's
 * bytes contiguous -- TcpServerTmpl::broadcast / foreachChannel
 * (evpp/TcpServer.h) for a batch, without the host reading the reply table,
 * walking the subscriptions and uploading a new table every turn.  What is
 * selected is the reply call's business and is not restated here: deferred
 * pieces, "close is final" and hvws_check's fail_rec apply as they do there
 * (run the reply call with HVWS_R_ECHO: its TEXT / BINARY replies are the
 * publications).
 *
 * Subscription table.  The caller's, in device memory, uploaded once
 * (hvws_h2d), kept across turns and changed on the device by
 * hvws_subs_update: topic t's subscribers are
 * d_member[d_topic_first[t] .. d_topic_first[t + 1]), ntopics + 1 words and
 * nmember ids.  A destination id is the caller's index of a connection in
 * [0, ndest), ndest <= 2^31 - 1; it need not be a segment of this batch (a
 * connection without a read still receives).  hvws_fanout itself never
 * changes the lists: hvws_subs_update (below) removes the connections the
 * reply call closed and applies the turn's joins and leaves, into the table
 * the next turn's hvws_fanout reads.  pub (host, nseg words, NULL = all
 * HVWS_FAN_NONE): the topic segment s publishes to; dest_of (host, nseg
 * words): segment s's own destination id.
 *
 * Edges.  R is the reply table, replies i = 0 .. nr - 1, op_i = flags & 0xF,
 * s_i the segment of the piece reply i answers.
 *   - op_i 1 or 2 is a publication.  With t = pub[s_i] not HVWS_FAN_NONE: one
 *     edge (i, j) per listing j of topic t, to destination
 *     d_member[d_topic_first[t] + j]; an edge to dest_of[s_i] is dropped unless
 *     HVWS_FAN_SELF is set; a destination listed twice is delivered twice.
 *     With t HVWS_FAN_NONE: no edges.
 *   - any other opcode (PONG, CLOSE): exactly one edge (i, 0), to dest_of[s_i].
 *
 * Output.  A dense table, one hvws_tx_msg per delivery, holding R[i] unchanged
 * (off / len still index the message call's d_out), sorted by the key
 * (destination, op_i == 8, i, j) ascending: a destination's deliveries are in
 * reply order -- sender order in the batch, then each sender's stream order --
 * and that destination's own CLOSE reply is its last frame.  reply[k] is the i
 * of delivery k; first[d] / count[d] destination d's range (a destination
 * without deliveries: the next destination's first, count 0).  After
 * hvws_send_messages(..., hvws_fanout_device, n, hvws_fanout_count_device, ...,
 * masked = 0, d_msg_off, ...) with n = *out_deliveries, destination d's bytes
 * are d_msg_off[first[d]] .. d_msg_off[first[d] + count[d]].
 * hvws_get_reply_flags of the reply call stays valid; for an HVWS_RF_FAILED
 * connection the host appends its 4-byte close behind dest_of[s]'s range.
 *
 * Waits once, as hvws_send_messages does: after the edge count the host reads
 * the delivery total E and the bad count, and writes *out_deliveries = E
 * (saturating).  HVWS_EINVAL, and the fanout getters then report none yet:
 *   - no preceding reply call, or a message call or a scan on ctx since it;
 *   - a flag bit other than HVWS_FAN_SELF; dest_of NULL or an entry >= ndest; a
 *     pub entry >= ntopics that is not HVWS_FAN_NONE; ndest 0 or above 2^31 - 1;
 *   - E > max_deliveries (*out_deliveries is still set), or more than 2^32 - 2
 *     edges counted before self edges are dropped;
 *   - a publication reaching a topic row with first[t] > first[t + 1] or
 *     first[t + 1] > nmember, or a member id >= ndest.  A bad row or id that no
 *     publication of the batch reaches is not looked at.
 * No read leaves d_topic_first[0 .. ntopics] or d_member[0 .. nmember).
 * Everything after the wait is asynchronous on the ctx stream;
 * hvws_last_kernel_ms reports the device work after the wait (expansion, sort,
 * finish) when this was the last call.  The tables are valid until the next
 * hvws_fanout, hvws_replies* or hvws_messages* on ctx; the getters
 * (hvws_fanout_device / hvws_fanout_count_device: d_msgs and d_n of
 * hvws_send_messages, NULL = none; hvws_fanout_count; hvws_get_fanout:
 * deliveries first .. first + n - 1 and the reply of each, either may be NULL;
 * hvws_get_dest_fanout: ndest entries each, either may be NULL) report none
 * after that, and the last two wait.  Results never depend on the kernels'
 * geometry and are the same on every run.   */
#define HVWS_FAN_NONE  UINT32_MAX
#define HVWS_FAN_SELF  1u     /* a sender that subscribes to its own topic gets its message too */
int hvws_fanout(hvws_ctx* ctx, const uint64_t* d_topic_first, const uint32_t* d_member, uint32_t ntopics,
                uint64_t nmember, uint32_t ndest, const uint32_t* pub, const uint32_t* dest_of, uint32_t flags,
                uint64_t max_deliveries, uint64_t* out_deliveries);
const hvws_tx_msg* hvws_fanout_device(hvws_ctx* ctx);
const uint64_t* hvws_fanout_count_device(hvws_ctx* ctx);
int64_t hvws_fanout_count(hvws_ctx* ctx);
int hvws_get_fanout(hvws_ctx* ctx, hvws_tx_msg* out, uint64_t* reply, uint64_t first, uint64_t n);
int hvws_get_dest_fanout(hvws_ctx* ctx, uint64_t* first, uint64_t* count);

/* ---- per-message topics and subscribe commands, device resident ------------- */
/* hvws_fanout takes one topic per connection for the whole batch, and
 * hvws_subs_update takes the joins and leaves from the host.  Where the clients
 * choose their topics -- a message names its room, "subscribe me to room 7"
 * arrives as a WebSocket message -- both need the message bytes, which are on
 * the device.  hvws_route reads the first bytes of every TEXT / BINARY reply of
 * the last hvws_replies / hvws_replies_checked where the message call left them
 * and leaves on the device a topic per REPLY, the reply rows with the command
 * header trimmed off, and the dense list of join / leave events;
 * hvws_fanout_routed is hvws_fanout reading those.  The reference has no
 * counterpart: its onmessage is user code.
 *
 * The command header.  A routed message, TEXT or BINARY alike, begins with one
 * header line of at most HVWS_ROUTE_HDR_MAX = 12 bytes:
 *     header = verb digits LF
 *     verb   = 'P' (0x50) | 'S' (0x53) | 'U' (0x55)
 *     digits = "0" | [1-9][0-9]{0,9}     decimal topic id, no sign, no leading zero
 *     LF     = 0x0A
 * With L the message length and h the header length (3 .. 12):
 *   - 'P': a publication to that topic.  The body is bytes [h, L) and may be
 *     empty; what is delivered is the body alone, with the reply's opcode and
 *     FIN (an ASCII line taken off the front of a valid UTF-8 text leaves it
 *     valid).
 *   - 'S' / 'U': subscribe / unsubscribe the sender; L must equal h.
 *   - everything else is malformed: L == 0; another verb (lowercase included);
 *     no digit; a leading zero; an eleventh digit; no LF within the first 12
 *     bytes or before the message ends ("P1\r\n" is malformed); a value >=
 *     ntopics, compared in 64 bits (ten digits exceed 2^32); 'S' / 'U' with
 *     bytes behind the LF.
 * Topic names instead of numbers (a hash table on the device) are out of scope:
 * names are the host's, numeric ids the device's.
 *
 * The rule, over the reply table R[0 .. nr) in table order, s_i the segment of
 * the piece reply i answers:
 *   - opcode other than 1 / 2 (PONG, CLOSE): kind HVWS_RK_OTHER, the row
 *     unchanged, topic HVWS_FAN_NONE.
 *   - opcode 1 / 2, parsed as above.  HVWS_RK_PUB: the row has off += h,
 *     len -= h, flags and key unchanged, topic[i] = the id.  HVWS_RK_SUB,
 *     HVWS_RK_UNSUB, HVWS_RK_BAD: the row unchanged, topic HVWS_FAN_NONE.
 *   - a malformed message fails its connection for this pass.  With b[s] the
 *     smallest reply index of kind BAD in segment s, every opcode-1 / 2 reply of
 *     s with index > b[s] has kind HVWS_RK_STOPPED whatever it holds (row
 *     unchanged, topic HVWS_FAN_NONE).  Neither BAD nor STOPPED replies deliver
 *     or produce an event; PONG and CLOSE replies of s are untouched (they are
 *     the reply call's business).  flags[s] gets HVWS_RT_BAD and bad_reply[s] =
 *     b[s], HVWS_ROUTE_NONE without one.  The host closes the connection (with
 *     1008, or what it likes) and passes it to hvws_subs_update as a DROP
 *     (hvws_subs_update_routed makes that DROP on the device).  In
 *     the RFC form a connection's data replies are in stream order, so b[s] is
 *     its first malformed message in the stream.
 *   - events: a dense table, one hvws_sub_event per SUB (HVWS_SUB_JOIN) and
 *     UNSUB (HVWS_SUB_LEAVE) reply, in reply order, {op, topic, dest_of[s_i]}:
 *     the array order hvws_subs_update applies.  A subscription therefore takes
 *     effect in the next turn's table, as that call documents.
 * The outputs are functions of the input alone: the same on every run, whatever
 * the kernels' geometry.
 *
 * hvws_route runs after hvws_replies / hvws_replies_checked, behind any of the
 * three message forms, is asynchronous on the ctx stream and does not wait;
 * hvws_last_kernel_ms reports it when it was the last call.  dest_of: host, nseg
 * words, segment s's own destination id.  It writes nothing the reply, message,
 * check or fan-out getters read: a plain hvws_fanout after it works on the
 * untouched reply table.  HVWS_EINVAL, nothing launched: no preceding reply
 * call, or a scan since it; dest_of NULL or an entry >= ndest; ndest 0 or above
 * 2^31 - 1; a reply capacity >= 2^32 - 1.  The message bytes are those of the
 * message call's d_out, which must still hold that call's output; no read
 * leaves [off, off + min(len, 12)) of a reply, nor [0, out_cap).  A deferred
 * piece is not in R and so is not routed.  The results are valid until the next
 * hvws_route, reply call, message call or scan on ctx; every getter reports
 * none after that (the _device ones NULL, hvws_route_event_count -1, the others
 * HVWS_EINVAL).  hvws_route_device: the routed rows, one per reply;
 * hvws_route_topics_device: the topic per reply; hvws_route_events_device /
 * hvws_route_event_count_device: the event table and its count.  These four do
 * not wait; the others do.  hvws_get_route: replies first .. first + n - 1, any
 * pointer may be NULL, a range beyond the reply count is HVWS_EINVAL;
 * hvws_get_route_events likewise over the events (what hvws_subs_update takes
 * as its host array: 12 B per event); hvws_get_route_flags: nseg entries each,
 * either may be NULL; hvws_get_route_totals: publications, subscribes,
 * unsubscribes, bad + stopped.
 *
 * hvws_fanout_routed follows hvws_fanout's contract word for word, except:
 * reply i's topic is topic[i] of the valid hvws_route on ctx, not pub[s_i]; the
 * rows delivered are the routed rows; ntopics, ndest and dest_of are that route
 * call's (none valid: HVWS_EINVAL); and since only the device knows which
 * replies publish, a NULL subscription table is refused whenever ntopics != 0.
 * A publication has one edge per listing of its topic, the self edge dropped
 * unless HVWS_FAN_SELF is set, a destination listed twice delivered twice;
 * PONG and CLOSE take one edge to the sender; SUB, UNSUB, BAD and STOPPED
 * replies have no edge; the sort key is (destination, op == 8, i, j); there is
 * one wait; the rules for bad rows and member ids apply only where a
 * publication reaches them.  It fills hvws_fanout's tables: every fan-out
 * getter (reply[k] is still the reply index), hvws_budget and
 * hvws_send_messages run behind it unchanged.   */
#define HVWS_ROUTE_HDR_MAX 12u
#define HVWS_RK_OTHER   0u   /* PONG, CLOSE: not parsed */
#define HVWS_RK_PUB     1u
#define HVWS_RK_SUB     2u
#define HVWS_RK_UNSUB   3u
#define HVWS_RK_BAD     4u   /* malformed */
#define HVWS_RK_STOPPED 5u   /* a data reply behind its connection's first malformed one */
#define HVWS_RT_BAD     1u   /* flags[s]: the connection sent a malformed message */
#define HVWS_ROUTE_NONE UINT64_MAX
int hvws_route(hvws_ctx* ctx, uint32_t ntopics, uint32_t ndest, const uint32_t* dest_of);
const hvws_tx_msg* hvws_route_device(hvws_ctx* ctx);
const uint32_t* hvws_route_topics_device(hvws_ctx* ctx);
const struct hvws_sub_event* hvws_route_events_device(hvws_ctx* ctx);
const uint64_t* hvws_route_event_count_device(hvws_ctx* ctx);
int hvws_get_route(hvws_ctx* ctx, hvws_tx_msg* rows, uint32_t* topic, uint8_t* kind, uint64_t first, uint64_t n);
int64_t hvws_route_event_count(hvws_ctx* ctx);
int hvws_get_route_events(hvws_ctx* ctx, struct hvws_sub_event* out, uint64_t first, uint64_t n);
int hvws_get_route_flags(hvws_ctx* ctx, uint8_t* flags, uint64_t* bad_reply);
int hvws_get_route_totals(hvws_ctx* ctx, uint64_t out[4]);
int hvws_fanout_routed(hvws_ctx* ctx, const uint64_t* d_topic_first, const uint32_t* d_member, uint64_t nmember,
                       uint32_t flags, uint64_t max_deliveries, uint64_t* out_deliveries);

/* ---- each topic's last message for joiners, device resident ----------------- */
/* A connection that subscribes to a topic hears nothing until someone publishes
 * there again; a feed or a room with state wants the last value at once (MQTT's
 * retained message, a last-value cache).  hvws_retain keeps each topic's most
 * recent publication in a store in device memory and leaves, for the turn's
 * subscribes, the rows a second hvws_send_messages sends from that store -- no
 * message byte, publication or subscribe command goes to the host.  The
 * reference has no counterpart: its onmessage is user code.
 *
 * The store is the caller's, in device memory, kept across turns and updated in
 * place: d_store holds ntopics slots of `slot` bytes, topic t's slot being
 * [t * slot, (t + 1) * slot), and d_ret holds ntopics entries.  ntopics, ndest
 * and dest_of are those of the valid hvws_route on ctx, as for
 * hvws_fanout_routed.  An entry counts as retained iff set == 1 and
 * 0 < len <= slot; anything else is "nothing retained", whatever the caller put
 * there.  The caller seeds both with hvws_memset to 0, or uploads values of its
 * own.
 *
 * The rule, over the routed replies i = 0 .. nr - 1 in table order:
 *   1. Update.  Of the replies of final kind HVWS_RK_PUB to topic t, the last
 *      (the largest i) wins; its trimmed body is [off, off + len) of the message
 *      call's d_out.
 *        - 0 < len <= slot: the body is copied to the front of slot t and
 *          d_ret[t] = {len, the routed row's flags, 1};
 *        - len == 0: d_ret[t] becomes all zero (an empty publication clears, as
 *          in MQTT);
 *        - len > slot: d_ret[t] becomes all zero and the topic is counted as
 *          oversize (a stale value is worse than none).
 *      A topic without a publication this turn is untouched: the update neither
 *      reads nor writes its entry or its slot.  BAD, STOPPED, SUB and UNSUB
 *      replies and PONG / CLOSE retain nothing.  Whether hvws_budget later cut a
 *      delivery does not matter: what was published is retained.
 *   2. Snapshot, taken after the update.  Every reply of final kind HVWS_RK_SUB
 *      (= every JOIN event of the route) whose topic t is retained produces one
 *      row {off = t * slot, len = d_ret[t].len, flags = d_ret[t].flags, key = 0}.
 *      The rows are dense and in reply order; topic[k] and reply[k] name row k's
 *      topic and SUB reply.  Replies are ordered by segment, so each segment's
 *      rows are contiguous: first[s] / count[s] (hvws_get_dest_fanout's
 *      convention for a segment without rows: the next segment's first, count
 *      0).  A subscription takes effect in the next turn's table, so with the
 *      snapshot taken after this turn's update a joiner misses nothing and gets
 *      nothing twice.  The device does not know who is a member already: a
 *      subscribe by a connection that is one gets a snapshot again.  A subscribe
 *      by a connection that also closes this turn still has its row; the caller
 *      does not write that connection's range.
 *   3. Send.  hvws_send_messages(ctx, d_tx2, cap2, d_store, ntopics * slot,
 *      hvws_retain_device(ctx), hvws_reply_capacity(ctx),
 *      hvws_retain_count_device(ctx), fragment, 0, d_msg_off2, ...) builds the
 *      snapshot frames; segment s's bytes are d_msg_off2[first[s]] ..
 *      d_msg_off2[first[s] + count[s]].  The caller writes them behind the
 *      connection's range of the turn's main send, and not at all for a
 *      connection the turn closed, failed or found malformed.  The snapshot is
 *      not under hvws_budget: the host holds its range against what byte_off
 *      left.
 * The outputs are functions of the input alone: the same on every run, whatever
 * the kernels' geometry; no atomic places a row or a byte.
 *
 * hvws_retain runs behind hvws_route, after any of the three message forms, is
 * asynchronous on the ctx stream and does not wait; hvws_last_kernel_ms reports
 * it when it was the last call.  The message call's d_out must still hold that
 * call's bytes.  It changes nothing the reply, route, fan-out, budget or subs
 * getters read and invalidates none of them: it may run anywhere behind the
 * route call.  HVWS_EINVAL, nothing launched and the store untouched: no valid
 * hvws_route on ctx; a flags bit set (none is defined); slot 0 or not a multiple
 * of 16, or ntopics * slot beyond 64 bits; with ntopics > 0, d_store or d_ret
 * NULL or d_store not 16-byte aligned; d_store[0, ntopics * slot), d_ret[0,
 * ntopics) and the message call's d_out[0, out_cap) overlapping one another.
 * Reads of a winning body stay inside [off, off + len) rounded outwards to 16
 * bytes and clipped to [0, out_cap); writes to d_store touch only [t * slot,
 * t * slot + len) of topics stored this turn; writes to d_ret only entries of
 * topics with a publication this turn; reads of d_ret only entries of topics
 * subscribed to and not published to this turn; nothing reads a slot.
 *
 * The snapshot tables are valid until the next hvws_retain, hvws_route, reply
 * call, message call or scan on ctx; every getter reports none after that (the
 * _device ones NULL, hvws_retain_count -1, the others HVWS_EINVAL).  The store
 * itself is the caller's and persists.  hvws_retain_device /
 * hvws_retain_count_device (d_msgs and d_n of hvws_send_messages; its n is
 * hvws_reply_capacity) do not wait; the others do.  hvws_get_retain: rows
 * first .. first + n - 1 with the topic and the SUB reply of each, any pointer
 * may be NULL, a range beyond the row count is HVWS_EINVAL;
 * hvws_get_segment_retain: nseg entries each, either may be NULL;
 * hvws_get_retain_totals: topics stored, cleared by an empty publication,
 * cleared by an oversize one, bytes copied, snapshot rows.  hvws_retain_tile:
 * the store bytes one workgroup of the copy covers per step (tests place body
 * lengths around it).   */
typedef struct hvws_retained {   /* 16 B per topic; all zero = nothing retained */
    uint64_t len;                /* bytes of the retained body in the topic's slot */
    uint32_t flags;              /* the routed row's flags (opcode, FIN) */
    uint32_t set;                /* 1 = a message is retained */
} hvws_retained;
int hvws_retain(hvws_ctx* ctx, uint8_t* d_store, uint64_t slot, hvws_retained* d_ret, uint32_t flags);
const hvws_tx_msg* hvws_retain_device(hvws_ctx* ctx);
const uint64_t* hvws_retain_count_device(hvws_ctx* ctx);
int64_t hvws_retain_count(hvws_ctx* ctx);
int hvws_get_retain(hvws_ctx* ctx, hvws_tx_msg* rows, uint32_t* topic, uint64_t* reply, uint64_t first, uint64_t n);
int hvws_get_segment_retain(hvws_ctx* ctx, uint64_t* first, uint64_t* count);
int hvws_get_retain_totals(hvws_ctx* ctx, uint64_t out[5]);
uint64_t hvws_retain_tile(void);

/* ---- deliveries that name their topic and sender, device resident ------------ */
/* hvws_route trims the command header off a publication: what is delivered is
 * the body alone, and a connection subscribed to two topics cannot tell which
 * one a message belongs to, nor who sent it.  hvws_envelope writes every
 * reply's outgoing bytes once into a second device buffer d_env, publications
 * with an envelope line in front, and leaves a row table R' over d_env, indexed
 * like the route's.  The fan-out, the budget and the send then run unchanged
 * over rows that point into d_env; no message byte goes to the host.  The
 * reference has no counterpart: its onmessage is user code.
 *
 * The envelope line mirrors the route's grammar:
 *   envelope = 'M' digits LF               flags == 0
 *            | 'M' digits SP digits LF     HVWS_ENV_SENDER
 *   digits   = "0" | [1-9][0-9]{0,9}
 * The first number is the reply's topic, the second dest_of[s_i] of the route
 * call, s_i being the connection the reply came from (4294967295 for a reply
 * whose piece is none of the batch's, which the fan-out refuses).  At most
 * HVWS_ENV_HDR_MAX bytes.  An ASCII line in front of valid UTF-8 leaves a TEXT
 * message valid UTF-8.
 *
 * The rule, over the valid route's replies i = 0 .. nr - 1 in table order:
 *   - HVWS_RK_PUB: reply i's bytes are the envelope (h'_i bytes) followed by
 *     the body, the routed row's [off, off + len) of the message call's d_out;
 *     R'[i] = {e_i, h'_i + len, flags, key}.  An empty body gives an envelope
 *     alone.
 *   - HVWS_RK_OTHER (PONG, CLOSE): the bytes are copied verbatim, at any
 *     length; R'[i] = {e_i, len, flags, key}.
 *   - SUB, UNSUB, BAD, STOPPED: no byte is written; R'[i] = {e_i, 0, flags,
 *     key}.  These replies have no edge in the fan-out.
 *   - e_0 = 0 and e_{i+1} = e_i + (bytes of reply i rounded up to 16): every
 *     reply starts 16-byte aligned, no 16-byte chunk of d_env belongs to two
 *     replies, and the pad bytes are never written.
 * The outputs are functions of the input alone: the same on every run, whatever
 * the kernels' geometry; no atomic places a row or a byte.
 *
 * Capacity.  hvws_envelope_bound(ctx) = out_cap + (HVWS_ENV_HDR_MAX + 15) *
 * hvws_reply_capacity(ctx) + 16 for the valid route on ctx (out_cap: the message
 * call's; 0 when it had no d_out), host arithmetic without a wait; 0 = no valid
 * route, or the sum exceeds 64 bits.  Replies answer disjoint pieces, so their
 * lengths sum to at most out_cap, and each adds at most 23 bytes of envelope
 * and 15 of padding.  There is no overflow path and no wait.
 *
 * hvws_envelope runs behind hvws_route, after any of the three message forms,
 * is asynchronous on the ctx stream and does not wait; hvws_last_kernel_ms
 * reports it when it was the last call.  The message call's d_out must still
 * hold that call's bytes.  It changes nothing the reply, route, fan-out, budget,
 * retain or subs getters read and invalidates none of them.  HVWS_EINVAL,
 * nothing launched and d_env untouched: no valid hvws_route on ctx; a flags bit
 * other than HVWS_ENV_SENDER; d_env NULL or not 16-byte aligned; env_cap below
 * hvws_envelope_bound; d_env[0, env_cap) overlapping the message call's
 * d_out[0, out_cap).  Reads of a body stay inside [off, off + len) rounded
 * outwards to 16 bytes and clipped to [0, out_cap); writes to d_env touch only
 * [e_i, e_i + bytes) of each reply.
 *
 * Its tables are valid until the next hvws_envelope, hvws_route, reply call,
 * message call or scan on ctx; every getter reports none after that
 * (hvws_envelope_device NULL, the others HVWS_EINVAL), and
 * hvws_fanout_enveloped / hvws_retain_enveloped are refused.  d_env itself is
 * the caller's.  hvws_envelope_device (one row per reply; hvws_reply_capacity
 * entries, hvws_reply_count of them written) does not wait; the others do.
 * hvws_get_envelope: rows first .. first + n - 1, a range beyond the reply count
 * is HVWS_EINVAL; hvws_get_envelope_totals: enveloped publications, replies
 * copied verbatim, bytes written, bytes of d_env spanned (e_nr).
 * hvws_envelope_tile: the bytes of d_env one workgroup of the copy covers per
 * step (tests place body lengths around it).
 *
 * hvws_fanout_enveloped follows hvws_fanout_routed's contract word for word,
 * except that the rows it delivers are R' and that it needs a valid
 * hvws_envelope on ctx (none: HVWS_EINVAL).  It fills hvws_fanout's tables:
 * every fan-out getter, hvws_budget, hvws_subs_update_routed and
 * hvws_send_messages run behind it unchanged; the send gets d_payload = d_env
 * and payload_len = env_cap, and the bound hvws_budget puts on a row's length
 * is env_cap in place of out_cap.
 *
 * hvws_retain_enveloped follows hvws_retain's contract word for word, except
 * that a winner's bytes are R'[i]'s bytes in d_env: a retained value is
 * envelope plus body, d_ret[t].len counts both, and a snapshot names its topic
 * by itself.  "Empty" still means an empty body (the routed row's len == 0);
 * oversize means h' + len > slot; the overlap rule covers d_env[0, env_cap) as
 * well as d_out; it needs a valid hvws_envelope on ctx and fills hvws_retain's
 * tables.  hvws_retain itself is unchanged (its flag bits stay refused).
 *  */
#define HVWS_ENV_SENDER  1u    /* the envelope names the publisher's destination id too */
#define HVWS_ENV_HDR_MAX 23u   /* 'M' + 10 digits + ' ' + 10 digits + LF */
uint64_t hvws_envelope_bound(hvws_ctx* ctx);
uint32_t hvws_envelope_tile(void);
int hvws_envelope(hvws_ctx* ctx, uint8_t* d_env, uint64_t env_cap, uint32_t flags);
const hvws_tx_msg* hvws_envelope_device(hvws_ctx* ctx);
int hvws_get_envelope(hvws_ctx* ctx, hvws_tx_msg* rows, uint64_t first, uint64_t n);
int hvws_get_envelope_totals(hvws_ctx* ctx, uint64_t out[4]);
int hvws_fanout_enveloped(hvws_ctx* ctx, const uint64_t* d_topic_first, const uint32_t* d_member, uint64_t nmember,
                          uint32_t flags, uint64_t max_deliveries, uint64_t* out_deliveries);
int hvws_retain_enveloped(hvws_ctx* ctx, uint8_t* d_store, uint64_t slot, hvws_retained* d_ret, uint32_t flags);

/* ---- per-topic sequence numbers in the envelope, device resident ------------- */
/* hvws_budget drops a slow destination's deliveries, and a snapshot of
 * hvws_retain cannot be related to the live deliveries that follow it: a
 * subscriber cannot tell that it missed a message.  hvws_sequence gives every
 * publication of the turn the next number of its topic's stream;
 * hvws_envelope_sequenced is hvws_envelope with that number on the line.  The
 * reference has no counterpart: its onmessage is user code.
 *
 * The counters.  d_seq is the caller's device memory, ntopics words of 8 bytes
 * (ntopics: the valid hvws_route's), kept across turns like hvws_retain's
 * d_ret.  d_seq[t] is the last number given out in topic t; the caller seeds it
 * (hvws_memset to 0, or its own values after a restart).
 *
 * The rule, over the valid route's replies i = 0 .. nr - 1 in table order:
 *   - a reply of kind HVWS_RK_PUB to topic t gets
 *       seq[i] = d_seq_before[t] + 1 + #{ j < i : kind[j] == PUB, topic[j] == t }
 *     modulo 2^64 (a counter at 2^64 - 1 gives 0 next);
 *   - after the call d_seq[t] = d_seq_before[t] + #{ PUB replies to t };
 *   - every other kind (OTHER, SUB, UNSUB, BAD, STOPPED) gets seq[i] = 0 and
 *     takes no number.  A PUB is told from the rest by its kind, not by
 *     seq != 0;
 *   - a topic without a publication this turn is neither read nor written;
 *   - numbers follow table order: behind hvws_messages_rfc each connection's
 *     stream order, connections in segment order;
 *   - whether hvws_budget later cuts a delivery does not matter: the hole that
 *     leaves in what a destination receives is the purpose.
 * The outputs are functions of the input alone: no atomic decides a number.
 *
 * hvws_sequence runs behind hvws_route, after any of the three message forms, is
 * asynchronous on the ctx stream and does not wait; hvws_last_kernel_ms reports
 * it when it was the last call.  It touches no payload byte, changes nothing the
 * reply, route, fan-out, budget, retain, envelope or subs getters read and
 * invalidates none of them.  It reads topic and kind per reply of the route and
 * d_seq[t] of the topics published to; it writes those d_seq[t] and its own
 * table.
 *
 * A turn is numbered once: a second hvws_sequence behind the same hvws_route is
 * HVWS_EINVAL and leaves the counters and the first call's table as they are (a
 * retry would skip numbers); the next hvws_route re-arms it.  HVWS_EINVAL,
 * nothing launched and the counters untouched, besides: no valid hvws_route on
 * ctx; a flags bit set (none is defined); with ntopics > 0, d_seq NULL or not
 * 8-byte aligned; d_seq[0, ntopics) overlapping the message call's
 * d_out[0, out_cap).  With ntopics == 0 the call succeeds and numbers nothing
 * (d_seq may be NULL).
 *
 * Its table is valid until the next hvws_sequence that is not refused as a
 * repeat, hvws_route, reply call, message call or scan on ctx; after that
 * hvws_sequence_device returns NULL, the getters HVWS_EINVAL, and
 * hvws_envelope_sequenced is refused.  hvws_sequence_device (seq per reply,
 * hvws_reply_capacity entries, 0 behind the reply count) does not wait; the
 * others do.  hvws_get_sequence: seq first .. first + n - 1, a range beyond the
 * reply count is HVWS_EINVAL; hvws_get_sequence_totals: publications numbered,
 * distinct topics published to.
 *
 * hvws_envelope_sequenced follows hvws_envelope's contract word for word --
 * offsets e_i, 16-byte alignment, verbatim PONG / CLOSE, rows of length 0 for
 * SUB / UNSUB / BAD / STOPPED, read and write bounds, the overlap rule, flags 0
 * or HVWS_ENV_SENDER -- except that
 *   - a publication's line carries its number:
 *       envelope = 'M' digits SP '#' seq LF              flags == 0
 *                | 'M' digits SP digits SP '#' seq LF    HVWS_ENV_SENDER
 *       seq      = "0" | [1-9][0-9]{0,19}
 *     seq being seq[i] of the valid hvws_sequence in decimal; at most
 *     HVWS_SEQ_HDR_MAX bytes.  The '#' keeps the two forms and hvws_envelope's
 *     own apart for a client's parser;
 *   - it needs a valid hvws_sequence on ctx (none: HVWS_EINVAL, d_env
 *     untouched);
 *   - env_cap is checked against hvws_envelope_sequenced_bound(ctx) = out_cap +
 *     (HVWS_SEQ_HDR_MAX + 15) * hvws_reply_capacity(ctx) + 16 (0 as
 *     hvws_envelope_bound);
 *   - it reads the number per reply besides.
 * It fills hvws_envelope's tables: hvws_envelope_device, hvws_get_envelope,
 * hvws_get_envelope_totals, hvws_fanout_enveloped and hvws_retain_enveloped,
 * and hvws_budget, hvws_subs_update_routed and hvws_send_messages behind them,
 * run unchanged.  A retained value is then line plus body: a snapshot tells the
 * joiner the number it holds, and the joiner expects that number + 1 next in the
 * topic.  hvws_envelope itself is unchanged (its other flag bits stay refused).
 *
 * Gap detection on the client.  A subscriber that saw n in a topic and then
 * n + 2 missed n + 1 -- unless n + 1 was its own publication: without
 * HVWS_FAN_SELF a publisher is not delivered its own messages, which take
 * numbers it does not otherwise see, and there is no acknowledgement row that
 * tells a publisher the number it was given.  A client that wants gap detection
 * must either be served with HVWS_FAN_SELF or learn from the application which
 * numbers its own publications took.   */
#define HVWS_SEQ_HDR_MAX 45u   /* 'M' + 10 digits + ' ' + 10 digits + ' ' + '#' + 20 digits + LF */
int hvws_sequence(hvws_ctx* ctx, uint64_t* d_seq, uint32_t flags);
const uint64_t* hvws_sequence_device(hvws_ctx* ctx);
int hvws_get_sequence(hvws_ctx* ctx, uint64_t* seq, uint64_t first, uint64_t n);
int hvws_get_sequence_totals(hvws_ctx* ctx, uint64_t out[2]);
uint64_t hvws_envelope_sequenced_bound(hvws_ctx* ctx);
int hvws_envelope_sequenced(hvws_ctx* ctx, uint8_t* d_env, uint64_t env_cap, uint32_t flags);

/* ---- per-destination write limits for the fan-out, device resident ---------- */
/* hvws_budget cuts every destination's deliveries of the last hvws_fanout at
 * the number of bytes that destination may still be sent, before a byte is
 * built: hio_write's rule (event/nio.c:554-560) -- a write whose unwritten bytes
 * would take the channel's write_bufsize above max_write_bufsize
 * (MAX_WRITE_BUFSIZE, 16 MiB, event/hevent.h:20; Channel::setMaxWriteBufsize,
 * evpp/Channel.h:178) fails with ERR_OVER_LIMIT and the channel is closed --
 * for the whole delivery table, without the host reading the table, sizing
 * every delivery, walking every range and uploading a filtered table.  It
 * runs between hvws_fanout and hvws_send_messages and does not wait.
 *
 * Input.  The last valid hvws_fanout on ctx (no reply or message call since,
 * and no scan since its reply call): its delivery table T[0 .. n), reply[] and
 * first[d] / count[d], ndest that call's.  d_budget: the caller's array in
 * device memory, ndest words, uploaded with hvws_h2d and kept across turns like
 * the subscription table; NULL: every destination's budget is budget_all
 * (ignored otherwise).  A budget is the bytes the destination may still be
 * sent -- its max_write_bufsize minus what its socket has queued; UINT64_MAX:
 * unlimited; every value is valid.  fragment and masked are those the
 * following hvws_send_messages will be given.
 *
 * Wire size.  w_k: the bytes hvws_send_messages emits for delivery k under that
 * fragment and masked -- websocket_calc_frame_size summed over the frames of
 * WebSocketChannel::send's fragmentation.
 *
 * Rule.  For destination d, over k = first[d] .. first[d] + count[d] - 1 in
 * table order, c_k = the sum of w_q over first[d] <= q <= k; delivery k is kept
 * iff c_k <= budget[d] (equality keeps it, as nio.c:556 does).  Sizes are
 * positive, so the kept deliveries are a prefix of the range: a destination
 * with a dropped delivery gets HVWS_BF_OVER, and nothing at or behind its first
 * dropped delivery goes out -- not a smaller delivery either, nor its own CLOSE
 * reply: the channel is closed.  A destination without deliveries is never
 * OVER; a budget of 0 drops everything.  One deviation: the reference applies
 * the check per write, that is per frame, so a fragmented message can be cut
 * between two fragments; this pass cuts at message boundaries -- a message
 * whose frames do not all fit is not started.  
 *
 * Output.  A dense table of the kept deliveries in the old order, hvws_tx_msg
 * rows unchanged; reply[k], the reply index of kept delivery k; the kept count
 * as a device word; per destination first[d] / count[d] in the new table
 * (hvws_get_dest_fanout's convention for a destination without deliveries),
 * flags[d], and byte_off, ndest + 1 words: the exclusive sum of the
 * destinations' kept wire bytes, its last word the total.  So after
 * hvws_send_messages(..., hvws_budget_device, n = hvws_fanout_count,
 * hvws_budget_count_device, fragment, masked, d_msg_off, ...) destination d's
 * bytes are byte_off[d] .. byte_off[d + 1], equal to d_msg_off[first[d]] ..
 * d_msg_off[first[d] + count[d]], and out[1] of the totals is that call's
 * exact *out_len: the out_cap to allocate.  The host closes the OVER
 * destinations and passes them to hvws_subs_update as HVWS_SUB_DROP events
 * (hvws_subs_update_routed with HVWS_SUBS_OVER makes them on the device).
 *
 * Asynchronous on the ctx stream, no wait; hvws_last_kernel_ms reports it when
 * it was the last call.  It writes nothing the fan-out's getters, the reply
 * call or the message call read: hvws_fanout_device stays valid beside it.
 * HVWS_EINVAL with nothing launched: no valid hvws_fanout; masked not 0 or 1;
 * (fan-out count) x (wire size of one message of the message call's out_cap
 * bytes under fragment / masked) does not fit 64 bits -- checked on the host,
 * so no device sum can wrap.  No read leaves d_budget[0 .. ndest).  The
 * results are valid until the next hvws_budget, hvws_fanout, hvws_replies*,
 * hvws_messages* or scan on ctx; the getters (hvws_budget_device /
 * hvws_budget_count_device: d_msgs and d_n of hvws_send_messages, NULL = none;
 * hvws_budget_count: the kept deliveries, -1 = none; hvws_get_budget: kept
 * deliveries first .. first + n - 1 and the reply of each, either may be NULL;
 * hvws_get_dest_budget: ndest entries each, ndest + 1 for byte_off, any may be
 * NULL; hvws_get_budget_totals: kept deliveries, kept bytes, dropped
 * deliveries, destinations over) report none after that, and all but the first
 * two wait.  Results never depend on the kernels' geometry and are the same on
 * every run.   */
#define HVWS_BF_OVER 1u   /* the destination's deliveries were cut: the host closes it (ERR_OVER_LIMIT) */
int hvws_budget(hvws_ctx* ctx, const uint64_t* d_budget, uint64_t budget_all, uint64_t fragment, int masked);
const hvws_tx_msg* hvws_budget_device(hvws_ctx* ctx);        /* d_msgs of hvws_send_messages */
const uint64_t*    hvws_budget_count_device(hvws_ctx* ctx);  /* its d_n; its n is hvws_fanout_count */
int64_t hvws_budget_count(hvws_ctx* ctx);                    /* kept deliveries; waits; -1: none */
int hvws_get_budget(hvws_ctx* ctx, hvws_tx_msg* out, uint64_t* reply, uint64_t first, uint64_t n);
int hvws_get_dest_budget(hvws_ctx* ctx, uint64_t* first, uint64_t* count, uint64_t* byte_off, uint8_t* flags);
int hvws_get_budget_totals(hvws_ctx* ctx, uint64_t out[4]);  /* kept deliveries, kept bytes, dropped deliveries, destinations over */

/* ---- the subscription table's upkeep, device resident ------------------------ */
/* hvws_subs_update builds the next subscription table of hvws_fanout from the
 * current one: the connections the last reply call closed are removed from
 * every list, and a list of join / leave / drop events is applied -- what the
 * reference's event loop does to its channel map (evpp/TcpServer.h) when a
 * channel closes, for a whole turn, without the host reading the reply flags,
 * rebuilding both arrays and uploading them.  The caller keeps two tables and
 * alternates them, as the message calls alternate d_out: this call reads
 * (d_topic_first, d_member) and writes (d_topic_first_out, d_member_out).
 *
 * The rule, stated sequentially.
 *   1. Start from the rows L[t] = d_member[d_topic_first[t] .. d_topic_first[t + 1]).
 *   2. dest_of (host, one word per segment of the last reply call, or NULL):
 *      for every segment s whose reply flags hold HVWS_RF_CLOSED (an
 *      HVWS_RF_FAILED connection carries it too), every listing of dest_of[s]
 *      is removed from every row.  This happens before any event, so an event
 *      that joins the same id again stands: the id may already belong to a new
 *      connection.  NULL: no such drops, and no reply call is needed.
 *   3. events (host, nev of them) in array order: HVWS_SUB_JOIN appends dest to
 *      L[topic] -- under HVWS_SUBS_UNIQUE only if the row does not list dest at
 *      that moment; HVWS_SUB_LEAVE removes every listing of dest from L[topic];
 *      HVWS_SUB_DROP removes every listing of dest from every row (topic is
 *      ignored).  HVWS_SUBS_UNIQUE does not remove duplicates the old table had.
 *   4. Output: a dense table over the same ntopics, d_topic_first_out[0] = 0 and
 *      d_topic_first_out[ntopics] = the new nmember.
 *   5. Order within row t: the surviving listings of the old row in their old
 *      order, then the surviving joined listings by destination id ascending,
 *      then event order.  (hvws_fanout's result does not depend on the order
 *      within a row; it is fixed so that the output is a function of the input.)
 * In closed form, with stamp 0 for an old listing, 1 for the drops of step 2
 * and e + 2 for event e: a listing survives iff no LEAVE of its (topic, dest)
 * and no DROP of its dest has a stamp at or above its own.
 *
 * Waits once, as hvws_fanout does: after the counting kernels the host reads
 * the new nmember, the counts and the bad flag, and writes *out_nmember.
 * HVWS_EINVAL, with nothing written to either output array and
 * hvws_subs_count then reporting none:
 *   - an event op outside 1 .. 3, a JOIN / LEAVE topic >= ntopics, an event dest
 *     >= ndest; a flag bit other than HVWS_SUBS_UNIQUE; ndest 0 or above
 *     2^31 - 1; nmember or nev above 2^32 - 2;
 *   - dest_of given without a preceding reply call, or with a scan on ctx since
 *     it; a dest_of[s] >= ndest;
 *   - an old table that is not dense -- d_topic_first[0] != 0, a decreasing pair,
 *     d_topic_first[ntopics] != nmember -- or a member id >= ndest: this pass
 *     reads the whole table, so every row counts (found on the device,
 *     reported after the wait);
 *   - a new nmember above member_cap (*out_nmember is still set);
 *   - a NULL table where one is needed (d_member may be NULL only with nmember
 *     0, d_member_out only with member_cap 0, events only with nev 0); an output
 *     array overlapping an input array or the other output; an output array
 *     that is not 16-byte aligned.
 * nev == 0 with dest_of NULL is a valid compacting copy.  No read leaves
 * d_topic_first[0 .. ntopics], d_member[0 .. nmember) or the reply call's
 * flags; no write touches d_member_out at or beyond the new nmember or
 * d_topic_first_out beyond ntopics + 1 words.  Everything after the wait is
 * asynchronous on the ctx stream; hvws_last_kernel_ms reports it (the
 * placement) when this was the last call.  The call neither reads nor
 * invalidates the message, reply or fanout tables: after the reply call a turn
 * may run hvws_fanout, hvws_send_messages and hvws_subs_update in any order.
 * hvws_subs_count: the new nmember of the last call (-1: none);
 * hvws_get_subs_counts: old listings kept, listings added, old listings
 * removed, distinct destinations dropped under step 2.  Results never depend
 * on the kernels' geometry and are the same on every run.   */
#define HVWS_SUB_JOIN   1u   /* append dest to topic's row */
#define HVWS_SUB_LEAVE  2u   /* remove every listing of dest from topic's row */
#define HVWS_SUB_DROP   3u   /* remove every listing of dest from every row; topic is ignored */
#define HVWS_SUBS_UNIQUE 1u  /* flags: a JOIN of a destination the row already lists adds nothing */
typedef struct hvws_sub_event { uint32_t op, topic, dest; } hvws_sub_event;   /* 12 B */
int hvws_subs_update(hvws_ctx* ctx, const uint64_t* d_topic_first, const uint32_t* d_member, uint32_t ntopics,
                     uint64_t nmember, uint32_t ndest, const hvws_sub_event* events, uint64_t nev,
                     const uint32_t* dest_of, uint32_t flags, uint64_t* d_topic_first_out, uint32_t* d_member_out,
                     uint64_t member_cap, uint64_t* out_nmember);
int64_t hvws_subs_count(hvws_ctx* ctx);
int hvws_get_subs_counts(hvws_ctx* ctx, uint64_t out[4]);

/* hvws_subs_update_routed is hvws_subs_update for a turn that ran hvws_route:
 * the turn's joins, leaves and drops are on the device already -- the route's
 * event table, the reply call's and the route's per-segment flags, the
 * budget's per-destination flags -- and this call merges them there with the
 * host's own events instead of the host reading all of them, building the DROPs
 * and sending the lot back up.  ntopics, ndest and dest_of are those of the
 * valid hvws_route on ctx, as for hvws_fanout_routed.
 *
 * The merged event array M is, in this order:
 *   1. the route's events, in its table order;
 *   2. one {HVWS_SUB_DROP, 0, dest_of[s]} for every segment s of the reply call
 *      whose reply flags hold HVWS_RF_CLOSED (a failed connection carries it) or
 *      whose route flags hold HVWS_RT_BAD -- in segment order, one per segment,
 *      duplicates not merged;
 *   3. with HVWS_SUBS_OVER, one {HVWS_SUB_DROP, 0, d} for every destination d
 *      whose flags in the valid hvws_budget on ctx hold HVWS_BF_OVER, d ascending;
 *   4. the caller's events[0 .. nev) in array order: the service's own decisions,
 *      and the JOIN of a new connection that took a closed id over.  They stand
 *      because they come last.
 * The result -- both output arrays, *out_nmember, hvws_subs_count and
 * hvws_get_subs_counts -- is exactly that of hvws_subs_update(ctx,
 * d_topic_first, d_member, ntopics, nmember, ndest, M, |M|, NULL,
 * flags & HVWS_SUBS_UNIQUE, ...).  The fourth count is therefore 0: there is no
 * step-2 drop, the closed connections are events.  A DROP kills every listing
 * with a stamp at or below its own, so (2) removes the old listings as step 2
 * would -- and the listings the same turn's route events added: a connection
 * that sends "S7\n" and a CLOSE in one read ends up listed nowhere, which the
 * step-2 drop of hvws_subs_update fed the route's events does not give (it
 * applies before every event).
 *
 * Waits twice: once for the merged count (40 bytes) behind the merge kernels --
 * the sort and rank areas are sized by it -- and once as hvws_subs_update does.
 * Everything else is asynchronous on the ctx stream; hvws_last_kernel_ms reports
 * the placement.  No event crosses to the host except the caller's own.
 * HVWS_EINVAL, with neither output array written and hvws_subs_count reporting
 * none: no valid hvws_route on ctx (a later route, reply, message call or scan
 * ends it); HVWS_SUBS_OVER without a valid hvws_budget on ctx, or with one whose
 * ndest is not the route's; a flag bit outside HVWS_SUBS_UNIQUE |
 * HVWS_SUBS_OVER; a host event with op outside 1 .. 3, a JOIN / LEAVE topic >=
 * ntopics or a dest >= ndest (checked before anything is launched); nmember or
 * |M| above 2^32 - 2; and everything hvws_subs_update refuses about the tables
 * (NULLs, overlap, alignment, a table that is not dense, a member id >= ndest, a
 * new nmember above member_cap with *out_nmember still set).  No read leaves
 * the route's, the reply call's or the budget's tables or the caller's table,
 * and the call invalidates none of them: it may run anywhere behind hvws_route,
 * with HVWS_SUBS_OVER behind hvws_budget.  hvws_get_subs_merged: the counts of
 * the four parts of M; hvws_get_subs_events: M[first .. first + n) (waits; a
 * range beyond |M| is HVWS_EINVAL).  Both are HVWS_EINVAL before any
 * hvws_subs_update_routed and after a plain hvws_subs_update.  M is a function
 * of the input: no atomic places an event.   */
#define HVWS_SUBS_OVER 2u   /* hvws_subs_update_routed only: drop the last hvws_budget's OVER destinations */
int hvws_subs_update_routed(hvws_ctx* ctx, const uint64_t* d_topic_first, const uint32_t* d_member, uint64_t nmember,
                            const hvws_sub_event* events, uint64_t nev, uint32_t flags,
                            uint64_t* d_topic_first_out, uint32_t* d_member_out, uint64_t member_cap,
                            uint64_t* out_nmember);
int hvws_get_subs_merged(hvws_ctx* ctx, uint64_t out[4]);   /* route events, connection drops, OVER drops, host events */
int hvws_get_subs_events(hvws_ctx* ctx, hvws_sub_event* out, uint64_t first, uint64_t n);  /* the merged array; waits */

/* Batches of at most `bytes` (default 64 MiB; each segment <= 1 MiB) take
 * the single-launch small-batch path inside hvws_rx_batch (and so inside
 * FeedRecvData / websocket_parser_execute); 0 restores the default, ~0
 * disables the path.  ctx NULL = the calling thread's context used by the
 * reference-API entry points.  Returns the previous limit.  Results are identical
 * either way; only latency differs. */
uint64_t hvws_set_small_batch_limit(hvws_ctx* ctx, uint64_t bytes);

/* Resident small-path worker.  The reference API's single calls -- FeedRecvData
 * and websocket_parser_execute on a read of <= 32 KiB, websocket_decode,
 * websocket_parser_decode and a masked websocket_build_frame of <= 32 KiB --
 * are served by one workgroup (k_door) that stays on the device between
 * calls and takes requests from a mailbox (in device memory written through
 * the PCIe BAR on large-BAR devices, else in pinned host memory): no kernel
 * launch per call.  It runs on a stream of its own (its own hardware queue)
 * and parks itself after $HVWS_DOOR_IDLE_US (default 5000) without a
 * request; the next call relaunches it.  Context teardown, thread exit and
 * process exit park it too.  on = 1 / 0 (off: each call launches k_small, or
 * the XOR kernel), -1 = default ($HVWS_DOOR, on unless set to 0).  ctx NULL = the
 * calling thread's context.  Returns the previous setting.  Results are
 * identical either way; only latency differs. */
int hvws_set_door(hvws_ctx* ctx, int on);
/* out = {worker launches, requests posted, requests the current worker
 * served, worker resident now} (tests, benchmarks). */
int hvws_door_stats(hvws_ctx* ctx, uint64_t out[4]);
/* Process-wide worker failures since the process started: out = {worker
 * streams that did not drain within 5 s (their context keeps the stream and
 * mailbox and never reuses them), requests a worker did not answer (that
 * context launches per call from then on)}.  Each is also reported on stderr
 * when it happens; both are 0 in a healthy process (the test session fails
 * otherwise).  At most $HVWS_DOOR_MAX (default 8) contexts per device hold a
 * worker stream at once; reads on further contexts launch per call. */
int hvws_door_health(uint64_t out[2]);
/* Idle time after which workers launched from now on park (microseconds;
 * 0 = the default, 5000).  Returns the previous value.  The runtime's frees
 * (hipFree, hipHostFree, hipHostUnregister) wait for every stream, a resident
 * worker's too: before each of its frees the library parks every worker on
 * that device, whichever thread owns it; a free outside this library waits
 * for the workers to park themselves (at most their idle time). */
uint64_t hvws_set_door_idle_us(uint64_t us);
/* Diagnostics for a process that seems stuck (bench.py's watchdog): writes
 * to fd the state of every context -- each resident worker's mailbox (seq,
 * done, alive, exited epoch) and the host's view of it, then
 * hipStreamQuery of every stream of the context (a query can itself block
 * behind a stuck runtime call; the memory state is written first).  The first
 * line ends with "holding D device bytes, P pinned bytes": what the library's
 * contexts hold in their grow-only buffers, process-wide -- a destroyed
 * context leaves neither behind. */
int hvws_debug_dump(int fd);
/* Diagnostics: a native backtrace of every thread of the process to fd
 * (SIGUSR2 to each thread in turn, backtrace_symbols_fd in the handler).
 * Returns the number of threads that answered within 200 ms each. */
int hvws_debug_backtraces(int fd);
/* out = {requests go through device memory written across the PCIe BAR (1)
 * or through pinned host memory (0), the context has a worker stream}. */
int hvws_door_info(hvws_ctx* ctx, uint64_t out[2]);
/* Diagnostics: 100 MHz device-clock stamps of the worker's last read request
 * -- seen, staged, walked, XORed, records written (before the release), and
 * the previous request's release.  Written only under $HVWS_EXPERIMENT
 * door_stamps=1 (each stamp costs the worker a clock round trip); else 0. */
int hvws_door_stamps(hvws_ctx* ctx, uint64_t out[12]);

/* Small batches whose segments are all <= 32 KiB (total <= 1 MiB; an event
 * loop's reads) are read by the device straight from pinned host memory, each
 * segment staged in LDS, with no H2D copy ahead of the launch (on = 1, the
 * default; $HVWS_SMALL_ZC=0 turns it off for new contexts).  ctx NULL = the
 * calling thread's context.  Returns the previous setting.  Results are
 * identical either way; only latency differs. */
int hvws_set_small_zero_copy(hvws_ctx* ctx, int on);

/* Registered pinned host memory: hvws_host_alloc'ed ranges are registered
 * automatically; hvws_host_register pins and registers caller memory (an
 * event loop's read buffers), hvws_host_unregister undoes it. */
int hvws_host_register(hvws_ctx* ctx, void* p, uint64_t bytes);
int hvws_host_unregister(hvws_ctx* ctx, void* p);

/* hvws_rx_batch over n separate reads that live in registered pinned memory
 * (no gather into a staging buffer, no copies: the kernel reads every read
 * where it is and unmasks it in place).  Each read is at most 32 KiB, the
 * total at most the small-batch limit (64 MiB by default), and reads must not
 * overlap.  Read i is segment i: hvws_get_segment_frames / hvws_get_frames
 * report its frames with hdr_off / pay_off relative to reads[i]; carry is
 * in/out per read.  HVWS_EINVAL (nothing done) if a read is not registered,
 * or if the context's small-batch path is off (hvws_set_small_batch_limit ~0). */
int hvws_rx_reads(hvws_ctx* ctx, char* const* reads, const uint64_t* lens, websocket_parser* carry, uint32_t n,
                  int unmask);

/* Host-inclusive streaming unmask of a large pinned host buffer holding
 * frames back to back from one stream: chunked H2D -> scan -> unmask -> D2H,
 * double-buffered over two streams.  carry is in/out. */
int hvws_pipeline(hvws_ctx* ctx, uint8_t* h_rx, uint64_t len, uint64_t chunk,
                  websocket_parser* carry);

/* ---- WebSocketParser handle for FFI ------------------------------------ */
typedef void (*hvws_msg_cb)(void* user, int opcode, const char* data, size_t len);
void* hvws_wsp_new(void);
void  hvws_wsp_free(void* h);
void  hvws_wsp_set_sink(void* h, hvws_msg_cb cb, void* user);
int   hvws_wsp_feed(void* h, const char* data, size_t len);
void  hvws_wsp_state(void* h, uint64_t out[8]);
/* n handles fed in one GPU round trip (see hvws_feed_many in WebSocketParser.h) */
int   hvws_wsp_feed_many(void* const* handles, const char* const* data, const size_t* len, int n, int* rets);

/* Pipelined event-loop feed.  A feeder owns a
 * worker thread with its own context, stream and pinned stage.  Each submit
 * starts the device half of this poll iteration's reads (gather, one GPU round
 * trip, unmasked bytes written back in place) on the worker and, meanwhile,
 * replays the PREVIOUS submission's message logic and onMessage callbacks on
 * the calling thread.  Effects per parser are those of hvws_feed_many, one
 * submission late: the callbacks and rets[] of submission k arrive during
 * submit k+1 (or flush).  The caller keeps submission k's buffers and its
 * rets array alive and untouched until then.  Submitting 0 reads = flush.
 * A parser whose feed returned short must be closed (as libhv does); its
 * results already in flight are then undefined.  Submit and flush are not
 * callable from inside the feeder's own callbacks (they return -1), nor may a
 * submission hold a parser that a replay still to come will write (see
 * hvws_feed_many; -1).  new() binds the calling thread's device; free()
 * flushes.  free() from inside one of the feeder's own callbacks is deferred:
 * the feeder is freed when the submit / flush that replays it returns (the
 * rest of that run's callbacks still run; runs of that submission not yet
 * started are dropped and its return value counts the reads taken). */
typedef struct hvws_feeder hvws_feeder;
hvws_feeder* hvws_feeder_new(void);
void hvws_feeder_free(hvws_feeder* f);
int  hvws_feeder_flush(hvws_feeder* f);
/* hvws_feeder_submit over hvws_wsp_* handles (C++: hvws_feeder_submit in WebSocketParser.h) */
int  hvws_wsp_feeder_submit(hvws_feeder* f, void* const* handles, const char* const* data, const size_t* len, int n,
                            int* rets);

/* Device used by the reference-API entry points on the calling thread
 * (default: $HVWS_DEVICE or 0). */
int hvws_set_thread_device(int device);
/* Free the calling thread's reference-API context (streams, device tables,
 * pinned staging); call at event-loop thread exit.  The next call on the
 * thread creates a fresh one. */
void hvws_thread_release(void);

#ifdef __cplusplus
}
#endif
#endif /* HVWS_H */
