// hvws_engine.cpp -- host side of the MI355X WebSocket receive engine:
// per-(thread, device) contexts, frame-table management, kernel sequencing,
// and the C ABI declared in include/hvws.h and include/hvws_synth.h.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dirent.h>
#include <immintrin.h>
#include <execinfo.h>
#include <signal.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <vector>
#include <mutex>
#include <shared_mutex>
#include <atomic>

#include "hvws.h"
#include "hvws_internal.h"
#include "hvws_synth.h"

using namespace hvws;

namespace {

thread_local char g_err[512] = "";

int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_OR(expr, code)                                                              \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return set_err((code), "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                           __LINE__);                                                   \
    } while (0)

// The runtime's frees (hipFree, hipHostFree, hipHostUnregister) wait for
// every stream of the device -- a resident k_door worker's too, until it
// parks.  Every free here first parks every worker on the current device,
// whichever thread owns it (defined with the worker).
void door_park_device();

// Device and pinned bytes currently held through dbuf / hbuf, process-wide
// (hvws_debug_dump prints them: a destroyed context leaves neither behind).
std::atomic<uint64_t> g_dev_bytes{0}, g_pin_bytes{0};

// Grow-only device allocation.
struct dbuf {
    void* p = nullptr;
    uint64_t cap = 0;
    hipError_t ensure(uint64_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        release();
        uint64_t want = std::max<uint64_t>(bytes + bytes / 2, 4096);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) g_dev_bytes += (cap = want);
        return e;
    }
    // ensure(), with a new allocation zeroed on st (arrays the kernels leave zero between uses)
    hipError_t ensure_zeroed(uint64_t bytes, hipStream_t st) {
        const void* was = p;
        const uint64_t had = cap;
        const hipError_t e = ensure(bytes);
        return e == hipSuccess && (p != was || cap != had) ? hipMemsetAsync(p, 0, cap, st) : e;
    }
    void release() {
        if (p) {
            door_park_device();
            hipFree(p);
            g_dev_bytes -= cap;
        }
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

struct hbuf {   // grow-only pinned host allocation
    void* p = nullptr;
    void* dev = nullptr;   // its device-mapped address, looked up once per allocation
    uint64_t cap = 0;
    unsigned flags = hipHostMallocDefault;   // hipHostMallocCoherent: device reads/writes bypass its caches
    hipError_t ensure(uint64_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        release();
        uint64_t want = std::max<uint64_t>(bytes + bytes / 2, 4096);
        hipError_t e = hipHostMalloc(&p, want, flags);
        if (e == hipSuccess) g_pin_bytes += (cap = want);
        return e;
    }
    void release() {
        if (p) {
            door_park_device();
            hipHostFree(p);
            g_pin_bytes -= cap;
        }
        p = nullptr;
        dev = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

void free_all(std::initializer_list<dbuf*> l) {
    for (dbuf* b : l) b->release();
}

// Which part of a context's memory a release() frees: hvws_ctx_destroy runs
// the device frees, then the pinned frees, then the event destroys.
enum rel { REL_DEVICE, REL_PINNED, REL_EVENTS };

// A pass's per-connection input on its way up: a pinned slot, reusable once
// the copy that read it has run (the event, created on first use), so a pass
// never waits for the previous pass's kernels.
struct up_slot {
    hbuf h;
    hipEvent_t ev = nullptr;
    bool pending = false;
    // a (na bytes), then b (nb bytes) behind it, to dst in one copy on st;
    // nothing at all without a or without bytes
    int send(void* dst, hipStream_t st, const void* a, uint64_t na, const void* b = nullptr, uint64_t nb = 0) {
        if (!a || !na) return HVWS_OK;
        if (!ev) HIP_OR(hipEventCreateWithFlags(&ev, hipEventDisableTiming), HVWS_EHIP);
        if (pending) {   // the previous pass's copy out of the slot
            HIP_OR(hipEventSynchronize(ev), HVWS_EHIP);
            pending = false;
        }
        HIP_OR(h.ensure(na + nb), HVWS_ENOMEM);
        memcpy(h.p, a, na);
        if (nb) memcpy(h.as<uint8_t>() + na, b, nb);
        HIP_OR(hipMemcpyAsync(dst, h.p, na + nb, hipMemcpyHostToDevice, st), HVWS_EHIP);
        HIP_OR(hipEventRecord(ev, st), HVWS_EHIP);
        pending = true;
        return HVWS_OK;
    }
    void release(rel ph) {
        if (ph == REL_PINNED) h.release();
        if (ph == REL_EVENTS && ev) {
            hipEventDestroy(ev);
            ev = nullptr;
        }
    }
};

}  // namespace

namespace hvws {
hvws_ctx* thread_ctx();
[[noreturn]] void fatal(const char* what);
}

static_assert(sizeof(drec) == sizeof(hvws_frame), "drec mirrors hvws_frame");
static_assert(sizeof(dsmall_out) == 64, "dsmall_out layout");

// What one scan produces (frame table, tile index, per-segment results and
// scratch); the context holds two.
struct tset {
    dbuf carry_out, counts, bases, total;
    dbuf sc_mid, sc_npred, sc_pbase, sc_fail, sc_masked, sc_total, sc_est;
    dbuf f_hdr, f_off, f_len, f_length, f_key, f_keyrot, f_info;
    dbuf tile_first, tile_key, tile_kind;
    dbuf runs, run_fail, run_trun;   // RUN path: per-segment run descriptors, failure words, per-tile records
    uint64_t frame_cap = 0;
    hipEvent_t free_ev = nullptr;   // recorded after the last kernel reading the set (pipelined steps)
    hipEvent_t free_wait = nullptr; // what the next scan into the set waits for: free_ev, or the stop
                                    // event attached to the unmask's own dispatch (no marker packet)
    bool free_pending = false;
    void release() {
        free_all({&carry_out, &counts, &bases, &total, &sc_mid, &sc_npred, &sc_pbase, &sc_fail, &sc_masked, &sc_total,
                  &sc_est, &f_hdr, &f_off, &f_len, &f_length, &f_key, &f_keyrot, &f_info, &tile_first, &tile_key,
                  &tile_kind, &runs, &run_fail, &run_trun});
        frame_cap = 0;
    }
};

// State of one table pass each (and of the transmit side): its device
// buffers, its upload slot, what its last call left.  release() lists exactly
// the members declared above it.

// hvws_utf8: per-record words and interior flags (zero between passes), its
// tile index, {record count}, per-segment state in / out and verdicts;
// state_in goes up through the slot.  gen: the scan (scan_gen) it ran over.
struct pass_u8 {
    dbuf words, flags, tiles, meta, in, out, bad;
    up_slot up;
    bool have = false;
    uint32_t nseg = 0;
    uint64_t gen = 0;
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&words, &flags, &tiles, &meta, &in, &out, &bad});
        up.release(ph);
    }
};

// hvws_messages: the scan's scratch, out_off per record, the tile index over
// the output, the piece table, per-segment first / count, state in / out,
// {records, payload bytes, pieces}; state_in goes up through the slot.
// hvws_messages_joined: the row table (length, source, key, info per row),
// each piece's last row, each segment's carry offset; prev_off goes up behind
// state_in in the same slot.
// hvws_messages_rfc: the class scan's scratch, each row's record, each
// virtual connection's carried row and record count; the states go up
// repacked (2 per connection, then their offsets: rf_st, rf_off) and come
// back as hvws_rfc_state in `out`.
struct pass_msg {
    dbuf scan, off, tiles, msgs, first, count, in, out, meta;
    dbuf row_len, row_src, row_key, row_info, prow, carry;
    dbuf cls, rec, vbase, vcnt;
    up_slot up;
    std::vector<hvws_msg_state> rf_st;
    std::vector<uint64_t> rf_off;
    bool have = false;
    bool joined = false;   // the last call was the joined form
    bool rfc = false;      // ... the RFC form
    uint32_t nseg = 0;
    uint64_t cap = 0;   // the piece bound of the last call (its record capacity; joined: its rows)
    uint64_t gen = 0;   // the scan it ran over
    uint64_t seq = 0;   // message calls so far
    const uint8_t* dout = nullptr;   // the last call's output and its capacity
    uint64_t out_cap = 0;
    void release(rel ph) {
        if (ph == REL_DEVICE)
            free_all({&scan, &off, &tiles, &msgs, &first, &count, &in, &out, &meta, &row_len, &row_src, &row_key,
                      &row_info, &prow, &carry, &cls, &rec, &vbase, &vcnt});
        up.release(ph);
    }
};

// hvws_send_messages: the message scan's scratch, each message's first frame,
// {frames, bytes, bad, count, uniform layout}, and the per-frame rows k_build
// reads (out_off and size in pass_tx's off / size)
struct pass_send {
    dbuf scan, first, meta, poff, len, flags, mask;
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&scan, &first, &meta, &poff, &len, &flags, &mask});
    }
};

// hvws_replies: the scan's scratch (word `cap` of it: the reply count), each
// segment's closing limit, the reply table and the piece each reply answers,
// per-segment first / count / flags; closed_in goes up through the slot
struct pass_replies {
    dbuf scan, limit, msgs, piece, first, count, flags, closed;
    up_slot up;
    bool have = false;
    uint32_t nseg = 0;
    uint64_t cap = 0;
    uint64_t gen = 0;   // the scans (scan_gen) before the last call
    uint64_t seq = 0;   // reply calls so far
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&scan, &limit, &msgs, &piece, &first, &count, &flags, &closed});
        up.release(ph);
    }
};

// hvws_fanout: the edge scan's scratch, dest_of and pub per segment (they go up
// through the slot in one copy), per segment {mark, self edges, bad}, {edges,
// deliveries, bad, replies}, the sort's two pair arrays (keys, then values) and
// its histograms, the delivery table and the reply of each delivery,
// per-destination first / count.  rep / msg: the reply call (pass_replies::seq)
// and the message call (pass_msg::seq) it expanded.  key_in: which of ping /
// pong holds the sorted keys (hvws_budget reads them).  maxlen: the bound on a
// row's length hvws_budget takes (hvws_fanout_enveloped: its env_cap).
struct pass_fan {
    dbuf scan, in, seg, meta, ping, pong, hist, msgs, reply, first, count;
    up_slot up;
    bool have = false;
    uint32_t ndest = 0;
    uint64_t n = 0;   // deliveries
    uint64_t rep = 0, msg = 0;
    uint64_t maxlen = 0;
    int key_in = 0;
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&scan, &in, &seg, &meta, &ping, &pong, &hist, &msgs, &reply, &first, &count});
        up.release(ph);
    }
};

// hvws_route: the count scan's scratch, dest_of per segment (it goes up through
// the slot), the routed rows, topic and kind per reply, bad_reply and flags per
// segment, the event table, {events, publications, subscribes, unsubscribes,
// bad + stopped}.  rep / msg / gen: the reply call, the message call and the
// scans it ran behind; ntopics / ndest: its arguments (hvws_fanout_routed
// takes them from here).
struct pass_route {
    dbuf scan, in, rows, topic, kind, bad, flags, ev, meta;
    up_slot up;
    bool have = false;
    uint32_t nseg = 0, ntopics = 0, ndest = 0;
    uint64_t rep = 0, msg = 0, gen = 0;
    uint64_t seq = 0;   // route calls so far
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&scan, &in, &rows, &topic, &kind, &bad, &flags, &ev, &meta});
        up.release(ph);
    }
};

// hvws_retain: the plan scan's scratch, the winner word per topic, the copy
// plan (four arrays in one buffer), the snapshot rows with the topic and the
// SUB reply of each, per-segment first / count, {snapshot rows, stored, cleared
// empty, cleared oversize, bytes copied, snapshot rows}.  Nothing goes up: no
// slot.  The store and its entries are the caller's.  route / rep / msg / gen:
// the route call (pass_route::seq), the reply call, the message call and the
// scans it ran behind.
struct pass_retain {
    dbuf scan, win, plan, rows, topic, reply, first, count, meta;
    bool have = false;
    uint32_t nseg = 0;
    uint64_t route = 0, rep = 0, msg = 0, gen = 0;
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&scan, &win, &plan, &rows, &topic, &reply, &first, &count, &meta});
    }
};

// hvws_envelope: the plan scan's scratch, the enveloped rows (and their twin
// for hvws_retain_enveloped), the copy plan (four arrays in one buffer),
// {enveloped publications, replies copied verbatim, bytes written, bytes of
// d_env spanned}.  Nothing goes up: no slot.  d_env is the caller's.  route /
// rep / msg / gen: the route call (pass_route::seq), the reply call, the message
// call and the scans it ran behind; env / env_cap / flags: its arguments.
struct pass_envelope {
    dbuf scan, rows, rrows, plan, meta;
    bool have = false;
    uint8_t* env = nullptr;
    uint64_t env_cap = 0;
    uint32_t flags = 0;
    uint64_t route = 0, rep = 0, msg = 0, gen = 0;
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&scan, &rows, &rrows, &plan, &meta});
    }
};

// hvws_sequence: the head scan's scratch, the sort's two pair arrays (keys,
// then values) and its histograms, the number per reply, {publications
// numbered, distinct topics published to}.  Nothing goes up: no slot.  The
// counters are the caller's.  route / rep / msg / gen: the route call
// (pass_route::seq), the reply call, the message call and the scans it ran
// behind.  numbered: the route call whose turn the counters last moved on for
// (0: none) -- a turn is numbered once.
struct pass_sequence {
    dbuf scan, ping, pong, hist, seq, meta;
    bool have = false;
    uint64_t route = 0, rep = 0, msg = 0, gen = 0;
    uint64_t numbered = 0;
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&scan, &ping, &pong, &hist, &seq, &meta});
    }
};

// hvws_budget: the size scan's scratch (the wire bytes before each delivery,
// the scans' scratch), per destination count2 / kept bytes / flags / first2 /
// byte_off, the kept table and the reply of each kept delivery, {kept
// deliveries, kept bytes, dropped deliveries, destinations over}.  Nothing
// per-connection goes up: no slot.  rep / msg: the pass_fan::rep / msg pair of
// the fan-out it ran over (hvws_fanout clears have), gen: the scans before it.
struct pass_budget {
    dbuf scan, cnt, kept, flags, first, off, msgs, reply, meta;
    bool have = false;
    uint32_t ndest = 0;
    uint64_t n = 0;   // the fan-out's deliveries
    uint64_t rep = 0, msg = 0, gen = 0;
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&scan, &cnt, &kept, &flags, &first, &off, &msgs, &reply, &meta});
    }
};

// hvws_subs_update: the events with dest_of behind them (they go up through
// the slot in one copy), the last drop stamp per destination, the sort's two
// pair arrays (keys, then values) and its histograms, the sorted events as
// (topic, destination) words, each topic's first of them, their ops / effective bits / "listed before"
// marks (a byte each), the old listings' survive bits, the row of every 256th
// listing, the ranks over the
// events and over the listings, {new nmember, kept, added, removed, dropped,
// bad} with the two counters behind them.  h: those counts on the host.
// hvws_subs_update_routed: the merged event array, the two compactions' ranks
// and scratch, {route events, connection drops, OVER drops, host events, their
// sum}.  merged: the last call was that one and its merge was read (m: those
// counts on the host).
struct pass_subs {
    dbuf in, drop, ping, pong, hist, pk, evfirst, bits, surv, brow, erank, lrank, meta;
    dbuf mev, mscan, mcnt;
    up_slot up;
    bool have = false;
    bool merged = false;
    uint64_t h[6] = {0, 0, 0, 0, 0, 0};
    uint64_t m[5] = {0, 0, 0, 0, 0};
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&in, &drop, &ping, &pong, &hist, &pk, &evfirst, &bits, &surv, &brow, &erank, &lrank,
                                        &meta, &mev, &mscan, &mcnt});
        up.release(ph);
    }
};

// hvws_check: the sequence scan's scratch, one byte of violation classes per
// record and piece, per-connection state in / out, fail_rec, why and code;
// state_in goes up through the slot.  msg: the message call (pass_msg::seq)
// it checked.
struct pass_check {
    dbuf scan, viol, in, out, fail, why, code;
    up_slot up;
    bool have = false;
    uint32_t nseg = 0;
    uint64_t msg = 0;
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&scan, &viol, &in, &out, &fail, &why, &code});
        up.release(ph);
    }
};

// transmit side (hvws_build_frames; hvws_send_messages reads its counts
// through h as well)
struct pass_tx {
    dbuf size, off, scan, tiles, stat, span;
    hbuf h;
    int variant = 0;        // k_build geometry of the last build
    bool uniform = false;   // ... and whether it built a uniform layout without a tile index
    void release(rel ph) {
        if (ph == REL_DEVICE) free_all({&size, &off, &scan, &tiles, &stat, &span});
        if (ph == REL_PINNED) h.release();
    }
};

struct hvws_ctx {
    int device = 0;
    hipStream_t stream = nullptr;    // compute
    hipStream_t copy_in = nullptr;   // pipeline H2D
    hipStream_t copy_out = nullptr;  // pipeline D2H
    // Pipelined steps (hvws_step_resident): discovery on sstream, overlapping
    // the previous batch's unmask on `stream`.  cs = the stream the current
    // scan enqueues on.
    hipStream_t sstream = nullptr;
    hipStream_t cs = nullptr;
    hipEvent_t scan_done = nullptr;
    bool piped = false;   // the last step was pipelined (set free events are being kept)
    // per-batch tables: the segment/carry tables the scan reads, and two
    // sets of everything a scan produces, used in turn, so a batch's scan
    // can run while the previous batch's unmask still reads its tables
    dbuf segs, carry_in;
    tset ts[2];
    int cur = 0;
    tset& T() { return ts[cur]; }
    hbuf h_segs, h_total;
    // Segment/carry upload staging: two pinned slots used in turn, each
    // reusable once the H2D copy that read it has run (event), so a step
    // never waits for the previous step's kernels.
    // The scan's first kernel reads the slot through its device mapping (no
    // copy); up_src_* point at the slot the next scan is to read.
    hbuf h_up[2];
    hipEvent_t up_ev[2] = {nullptr, nullptr};
    bool up_pending[2] = {false, false};
    int up_next = 0;
    int up_slot = -1;
    const dseg* up_src_segs = nullptr;
    const dcarry* up_src_carry = nullptr;
    // Speculative EMIT (SCAN_SPEC): per-segment estimates, the device's
    // verdict in pinned memory, and whether the last exact scan says the
    // estimates hold (then the next batch speculates).
    hbuf h_status;
    uint64_t scan_seq = 0;
    bool spec_ok = false;
    // The last check saw a segment with >= spec_min predicted frames: the
    // next one-walk pass keeps the grid-wide k_verify pair (else head + walk).
    bool verify_hint = true;
    int verify_mode = -1;   // hvws_set_walk_verify: -1 adaptive (the hint), 0 never, 1 always
    int spec_mode = -1;   // -1 auto, 0 never, 1 SPEC first, 2 SLACK first ($HVWS_EXPERIMENT spec / hvws_set_speculation)
    // SLACK (mixed sizes, several segments): scratch table, exact bases, and
    // the per-segment region cap from the last exact scan's largest segment
    dbuf sl_hdr, sl_off, sl_len, sl_length, sl_key, sl_keyrot, sl_info, sl_bx;
    uint64_t sl_cap = 0;       // records the scratch table holds
    uint64_t slack_seg = 0;    // largest per-segment count of the last exact scan (0 = unknown)
    uint64_t fast_bound = 0;   // record bound below which COUNT -> EMIT needs no host wait; 0 = default
    int scan_path = -1;        // HVWS_PATH_* of the last scan
    int prev_path = -1;        // ... and of the one before (set when a scan starts)
    uint64_t single_hint = 0;  // records of the last one-segment scan whose count was read
    // RUN path (hvws_internal.h, drun): the last scan left no frame table (its
    // records are built on demand), its unmask is k_unmask_run + k_run_fix
    bool run_active = false;
    bool materializing = false;   // run_materialize's exact scan: no timing slot, no RUN bookkeeping
    bool run_call = false;     // the scan belongs to a step call (the only callers RUN serves)
    int run_mode = -1;         // hvws_set_run: -1 auto, 0 never, 1 whenever a step's batch allows it
    uint32_t run_skip = 0;     // steps left before RUN is tried again after a failed hypothesis
    uint64_t run_seq = 0;      // the current RUN step's verdict number
    uint64_t run_seen = 0;     // the last verdict read (dspec_status::run_seq)
    uint32_t run_vmask = 0;    // validation classes in force when the current RUN step ran (run_materialize)
    uint64_t last_mean = 0;    // bytes per record of the last exact (or SPEC) scan: RUN is for small frames
    // frame sieve (hvws_sieve.hip): one long mixed-size segment discovered in
    // parallel.  h_sv receives the device state + survivor and chain counts
    // after each sieved scan (read as hints by the next one).
    dbuf sv_state, sv_tcount, sv_tbase, sv_slot, sv_pool, sv_keep, sv_kbase, sv_Spre, sv_S, sv_J0, sv_J1, sv_mark, sv_hops, sv_rank, sv_cnt, sv_tmp, sv_scr;
    uint64_t sv_cap = 0, sv_capc = 0;
    uint64_t sv_hint_pre = 0, sv_hint_surv = 0;   // counts of the latest sieved scan read back
    hbuf h_sv;
    uint32_t sv_skip = 0;      // one-stream scans left before the sieve is tried again on uniform traffic
    bool sv_ran = false;       // the last scan launched the sieve
    hipEvent_t sv_ev = nullptr;   // h_sv holds the last sieved scan's state once this has completed
    uint64_t sv_gen = 0;       // sieve_generation() the history below belongs to
    uint64_t sv_win_len = 0;   // segment length of the last sieved scan if it sieved windows only, else 0
    uint32_t sv_full_left = 0; // scans left that sieve every tile (a windowed chain fell short)
    uint32_t sv_rt = 0, sv_wt = 0;   // window geometry of the last sieved scan (tiles)
    bool sv_hint_win = false;  // sv_hint_* come from a windowed scan
    uint64_t sv_mean = 0;      // bytes per frame along the last sieved chain (0: none yet)
    // hvws_pipeline: its three device slots and their events, kept across
    // calls (a per-call hipMalloc/hipFree pair cost the first call ~2x)
    dbuf pipe_slot[3], pipe_segs;
    hipEvent_t pipe_ev[9] = {};
    // staging for host-memory entry points
    dbuf stage;
    dbuf xor_stage;
    dbuf synth_sizes, synth_tiles, synth_bad;
    // The table passes behind a scan, and the transmit side: one struct each
    // (pass_u8 .. pass_tx above), which declares the pass's buffers and
    // releases them.  scan_gen counts the scans of the context.
    pass_u8 u8;
    pass_msg mg;
    pass_send sd;
    pass_replies rp;
    pass_fan fan;
    pass_route rt;
    pass_retain rn;
    pass_envelope en;
    pass_sequence sq;
    pass_budget bg;
    pass_subs subs;
    pass_check ck;
    pass_tx tx;
    uint64_t scan_gen = 0;
    bool ev_build = false;   // ev[4] .. ev[5] hold a timed region (hvws_last_kernel_ms)
    // small-batch path (k_small): upload packet, record slots, pinned results
    hbuf h_small_in, h_small_out;
    hbuf h_small_done;             // per-segment completion words k_small writes last
    uint64_t small_seq = 0;        // value the current call's completion words carry
    int small_poll = 1;            // $HVWS_EXPERIMENT small_poll: poll those words instead of syncing the stream
    bool small_quiet = false;      // the last small call saw all its words: its kernel no longer touches the pinned buffers
    hbuf h_feed;   // hvws_feed_many's gather buffer (reference-API thread contexts)
    dbuf d_small_in, d_small_slots;
    uint64_t small_limit = 0;   // bytes; 0 = default
    // k_small's record counter lives on the device and only ever grows; a
    // call's records start at small_ctr_base
    dbuf d_small_ctr;
    uint64_t small_ctr_base = 0;
    bool small_ctr_dirty = true;   // unknown value (first use, failed call): zero it
    int small_zc = 1;              // $HVWS_EXPERIMENT small_zc / hvws_set_small_zero_copy
    uint64_t zc_batch = kZcBatch;  // largest zero-copy batch ($HVWS_EXPERIMENT zc_batch)
    uint32_t vmask = 0;         // protocol validation classes (V_*); 0 = reference behaviour
    // last scan
    uint32_t nseg = 0;
    uint64_t nfr = 0;
    uint64_t rx_len = 0;
    const uint8_t* rx = nullptr;
    bool have_scan = false;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [4], [5]: build / keys
    // Per-step timing: scan begin/end and unmask begin/end events for the
    // last kTimeRing steps, read after the fact (hvws_step_times) so a caller
    // timing many steps need not synchronise after each.
    static constexpr int kTimeRing = 32;
    hipEvent_t tev[kTimeRing][4] = {};
    bool t_unmask[kTimeRing] = {};
    uint8_t t_rec[kTimeRing] = {};      // which of the slot's 4 events were recorded (bit i)
    uint64_t t_seq = 0;   // scans recorded so far
    int t_cur = 0;        // ring slot of the last scan
    uint32_t t_every = 1; // hvws_set_step_event_interval: events on every t_every-th scan (0: none)
    bool t_on = true;     // the current scan is one of them
    // resident small-path worker (k_door): its own HSA queue (a dedicated
    // hardware queue, so the resident kernel never holds up other work;
    // hvws_doorq.cpp), the mailbox, the data and record areas (fine-grained
    // pinned) and a device slot for records past the worker's LDS area
    door_queue* door_q = nullptr;
    hbuf h_door, h_door_data, h_door_rec;
    dbuf d_door_slot;
    // Request block + request bytes in fine-grained device memory, written by
    // the host through the PCIe BAR (round 4): the worker polls and stages
    // from its own HBM instead of pulling them across the link.  nullptr: the
    // request and its bytes go through the pinned box and data area (round 3).
    void* d_door_req = nullptr;
    bool door_live = false;     // launched and not yet seen to have ended
    bool door_wedged = false;   // its launch ran on past every bound: queue and mailbox are left alone
    bool door_broken = false;   // a request went unanswered: this context launches per call from now on
    // The HIP runtime call this context's worker lifecycle or teardown is
    // in (nullptr: none): a wedge report or hvws_debug_dump names the call.
    std::atomic<const char*> at{nullptr};
    uint64_t door_seq = 0;      // last request number posted
    uint64_t door_epoch = 0;    // launches so far; the worker writes its epoch to `exited` as it ends
    std::mutex door_m;          // one caller at a time: the owning thread, a free on another thread, exit
    int door_mode = -1;         // hvws_set_door: -1 default ($HVWS_DOOR, on), 0 off, 1 on
    uint64_t door_launches = 0, door_calls = 0;
    // hvws_span_begin / hvws_span_end: a timed region's begin and end markers
    // on both of the context's compute streams
    hipEvent_t span_ev[4] = {};
    int variant = 0;   // k_unmask geometry the tile index was built for
    bool nfr_known = false;   // else c->nfr is an upper bound, the count is on the device
    // table invariant check (hvws_set_table_checks)
    dbuf chk;
    hbuf h_chk;
    // host copy of the last scan's results (readback_all)
    hbuf h_readback;
    bool hcache_valid = false;
    std::vector<hvws_frame> hcache;
    std::vector<uint64_t> hfirst, hcount;
    std::vector<dcarry> hcarry;
};

namespace {
constexpr uint64_t kFastFrameBound = 1ull << 24;   // records: table sized by the bound, no count sync
constexpr uint64_t kReadbackPrefix = 1ull << 16;   // records read back speculatively with the rest
constexpr uint64_t kSingleMin = 1ull << 20;   // records: smallest one-stream table before its count is known
constexpr uint64_t kSlackMaxRecords = 1ull << 26;   // SLACK scratch table at most (48 B each: 3.2 GB)
// Small-batch path (k_small): batches up to kSmallBatch bytes whose segments
// are each at most kSmallSegment bytes run as one launch.
constexpr uint64_t kSmallBatch = 64ull << 20;
constexpr uint64_t kSmallSegment = 1ull << 20;
constexpr uint64_t kSmallHostRecords = 1ull << 20;   // records returned through pinned memory
int g_table_checks = -1;   // -1: from $HVWS_CHECK_TABLES on first use
bool table_checks() {
    if (__atomic_load_n(&g_table_checks, __ATOMIC_RELAXED) < 0) {
        const char* e = getenv("HVWS_CHECK_TABLES");
        int want = e && atoi(e) ? 1 : 0, unset = -1;
        __atomic_compare_exchange_n(&g_table_checks, &unset, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    }
    return __atomic_load_n(&g_table_checks, __ATOMIC_RELAXED) > 0;
}
}  // namespace

namespace {

dframes frames_of(hvws_ctx* c) {
    tset& t = c->T();
    return {t.f_hdr.as<int64_t>(), t.f_off.as<uint64_t>(), t.f_len.as<uint64_t>(), t.f_length.as<uint64_t>(),
            t.f_key.as<uint32_t>(), t.f_keyrot.as<uint32_t>(), t.f_info.as<uint32_t>(), t.frame_cap};
}

hipError_t ensure_frames(hvws_ctx* c, uint64_t n, bool exact = false) {
    if (n <= c->T().frame_cap && c->T().f_off.p) return hipSuccess;
    uint64_t want = std::max<uint64_t>(exact ? n : n + n / 4, 1024);
    hipError_t e;
    tset& t = c->T();
    for (dbuf* b : {&t.f_hdr, &t.f_off, &t.f_len, &t.f_length})
        if ((e = b->ensure(want * 8)) != hipSuccess) return e;
    for (dbuf* b : {&t.f_key, &t.f_keyrot, &t.f_info})
        if ((e = b->ensure(want * 4)) != hipSuccess) return e;
    t.frame_cap = want;
    return hipSuccess;
}

void to_dcarry(const websocket_parser& p, dcarry& d) {
    d.state = p.state;
    d.flags = (uint32_t)p.flags;
    memcpy(&d.mask, p.mask, 4);
    d.mask_offset = p.mask_offset;
    d.length = p.length;
    d.require = p.require;
    d.offset = p.offset;
    d.started = 0;
    // Validation state of a partial header lives in the struct's padding
    // byte after mask_offset (offset 13), invisible to the reference API.
    d.viol = reinterpret_cast<const uint8_t*>(&p)[kViolByte];
}

void from_dcarry(const dcarry& d, websocket_parser& p) {
    p.state = d.state;
    p.flags = (websocket_flags)d.flags;
    memcpy(p.mask, &d.mask, 4);
    p.mask_offset = (uint8_t)d.mask_offset;
    p.length = d.length;
    p.require = d.require;
    p.offset = d.offset;
    reinterpret_cast<uint8_t*>(&p)[kViolByte] = (uint8_t)d.viol;
}

int check_ctx(hvws_ctx* c) {
    if (!c) return set_err(HVWS_EINVAL, "null context");
    HIP_OR(hipSetDevice(c->device), HVWS_EHIP);
    return HVWS_OK;
}

// ... and the batch arguments of hvws_scan / hvws_step / hvws_step_resident.
int check_batch_args(hvws_ctx* c, const uint8_t* d_rx, const hvws_segment* segs, uint32_t nseg) {
    if (int rc = check_ctx(c)) return rc;
    if (!segs && nseg) return set_err(HVWS_EINVAL, "null segment table");
    if (((uintptr_t)d_rx & 15u) != 0) return set_err(HVWS_EINVAL, "rx buffer must be 16-byte aligned");
    return HVWS_OK;
}

// ---- what the table passes behind a scan share (hvws_utf8, messages_pass, hvws_check, ...)

// `who` runs over the last scan's tables: there is one, of this very buffer.
int behind_scan(hvws_ctx* c, const char* who, const uint8_t* d_rx, uint64_t rx_len) {
    if (!c->have_scan) return set_err(HVWS_EINVAL, "%s without a preceding hvws_scan", who);
    if (!d_rx || d_rx != c->rx || rx_len != c->rx_len)
        return set_err(HVWS_EINVAL, "%s buffer differs from the scanned one", who);
    return HVWS_OK;
}

// Records a pass sizes its tables for: c->nfr is the record count, or its
// bound while the count is on the device.
uint64_t record_bound(hvws_ctx* c) { return std::min<uint64_t>(c->nfr, c->T().frame_cap); }

// The device work hvws_last_kernel_ms times: between these two.
hipError_t timed_begin(hvws_ctx* c) { return hipEventRecord(c->ev[4], c->stream); }
hipError_t timed_end(hvws_ctx* c) {
    const hipError_t e = hipEventRecord(c->ev[5], c->stream);
    if (e == hipSuccess) c->ev_build = true;
    return e;
}

// Pipelined steps: the scan two steps on writes the current table set and
// must wait for the pass queued so far as it waits for the set's unmask.
hipError_t hold_tables(hvws_ctx* c) {
    if (!c->piped) return hipSuccess;
    tset& t = c->T();
    const hipError_t e = hipEventRecord(t.free_ev, c->stream);
    if (e != hipSuccess) return e;
    t.free_wait = t.free_ev;
    t.free_pending = true;
    return hipSuccess;
}

// Rows to the host on the context stream -- a null dst or no bytes: skipped --
// then one wait.
struct d2h_row {
    void* dst;
    const void* src;
    uint64_t bytes;
};
int read_rows(hvws_ctx* c, std::initializer_list<d2h_row> rows) {
    for (const d2h_row& r : rows)
        if (r.dst && r.bytes)
            HIP_OR(hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost, c->stream), HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    return HVWS_OK;
}

// One device word to the host; waits.
hipError_t read_word(hvws_ctx* c, const uint64_t* src, uint64_t* v) {
    const hipError_t e = hipMemcpyAsync(v, src, 8, hipMemcpyDeviceToHost, c->stream);
    return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

// ... as the count `who` returns: -1, and the error set, when the read fails
int64_t read_count(hvws_ctx* c, const uint64_t* src, const char* who) {
    uint64_t n = 0;
    if (read_word(c, src, &n) == hipSuccess) return (int64_t)n;
    set_err(HVWS_EHIP, "%s: reading the count failed", who);
    return -1;
}

// Device address of a pinned host buffer.
template <typename T>
T* mapped(hbuf& b) {
    if (!b.dev && b.p && hipHostGetDevicePointer(&b.dev, b.p, 0) != hipSuccess) b.dev = nullptr;
    return reinterpret_cast<T*>(b.dev);
}

// Which per-step timing events are recorded: 2 = scan begin/end and unmask
// begin/end, 1 = the unmask's only, 0 = none.  Default: 2 for serial steps,
// 1 for pipelined ones (hvws_step_resident) -- each timing marker is a packet
// the command processor runs between kernels, and the scan-side pair cost a
// pipelined c2 step ~9 us (0.465 -> 0.456 ms, profiles/r2d_raw); a pipelined
// scan's span includes its wait for the previous unmask anyway.
// $HVWS_EXPERIMENT step_events forces a mode.
int step_events(const hvws_ctx* c) {
    static const int v = [] {
        const char* e = experiment("step_events");
        return e ? atoi(e) : -1;
    }();
    return v >= 0 ? v : (c->cs != c->stream ? 1 : 2);
}

// Record timing event i (0 scan begin, 1 scan end, 2 unmask begin, 3 unmask
// end) of the current ring slot if this mode keeps it.
hipError_t tev_record(hvws_ctx* c, int i, hipStream_t st) {
    const int m = step_events(c);
    if (!c->t_on || m <= 0 || (m == 1 && i < 2)) return hipSuccess;
    c->t_rec[c->t_cur] |= (uint8_t)(1u << i);
    return hipEventRecord(c->tev[c->t_cur][i], st);
}

// Next slot of the timing ring: record the scan-begin event there (unless
// the caller attaches the slot's events to a dispatch itself).
hipError_t begin_timed_scan(hvws_ctx* c, bool record = true) {
    c->t_cur = (int)(c->t_seq % hvws_ctx::kTimeRing);
    c->t_unmask[c->t_cur] = false;
    c->t_rec[c->t_cur] = 0;
    c->t_on = c->t_every != 0 && c->t_seq % c->t_every == 0;
    ++c->t_seq;
    return record ? tev_record(c, 0, c->cs) : hipSuccess;
}

// out[0] = scan ms, out[1] = unmask ms (-1: no unmask, or not recorded) of
// the step in ring `slot`.
int step_times_at(hvws_ctx* c, int slot, float* out) {
    hipEvent_t* e = c->tev[slot];
    const uint8_t r = c->t_rec[slot];
    out[0] = out[1] = -1.0f;
    if ((r & 3u) == 3u) {
        HIP_OR(hipEventSynchronize(e[1]), HVWS_EHIP);
        HIP_OR(hipEventElapsedTime(&out[0], e[0], e[1]), HVWS_EHIP);
    }
    if (c->t_unmask[slot] && (r & 4u) && (r & 8u)) {
        HIP_OR(hipEventSynchronize(e[3]), HVWS_EHIP);
        HIP_OR(hipEventElapsedTime(&out[1], e[2], e[3]), HVWS_EHIP);
    }
    return HVWS_OK;
}

// $HVWS_RUN=0: the RUN path off (A/B runs); hvws_set_run overrides per context.
bool run_env() {
    static const int v = getenv("HVWS_RUN") ? atoi(getenv("HVWS_RUN")) : 1;
    return v != 0;
}

// Wait until k_spec_check has published scan `seq` in the (fine-grained)
// pinned status: the device stores it with system-scope release as its last
// write, so the host polls it instead of a stream event (an event marker
// costs ~10 us of device idle between the check and the tile kernels).  A
// stream that drains without publishing is an error, never a hang.
// tiles: wait for tseq instead, published after the scan's last kernel
// (launch_publish_tiles) -- pipelined SPEC and RUN steps queue the unmask
// once the host has seen it, not behind a cross-stream event.
int wait_status(hvws_ctx* c, uint64_t seq, bool tiles = false) {
    const dspec_status* st = c->h_status.as<dspec_status>();
    const uint64_t* w = tiles ? &st->tseq : &st->seq;
    for (uint64_t spin = 0;; ++spin) {
        if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq) return HVWS_OK;
        if ((spin & 1023) == 1023) {
            const hipError_t q = hipStreamQuery(c->cs);
            if (q == hipSuccess) {
                if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq) return HVWS_OK;
                return set_err(HVWS_EHIP, "scan check did not publish (seq %llu)", (unsigned long long)seq);
            }
            if (q != hipErrorNotReady) return set_err(HVWS_EHIP, "stream error: %s", hipGetErrorString(q));
        }
        __builtin_ia32_pause();
    }
}

// The last sieved scan's state has landed in h_sv.
bool sieve_state_ready(hvws_ctx* c) { return c->sv_ran && c->sv_ev && hipEventQuery(c->sv_ev) == hipSuccess; }

// Frame-sieve buffers for a one-segment scan of rx_len bytes.  The survivor
// capacity is sized from the batch (one survivor per KiB) and from the last
// sieved scan's survivor count; a batch with more survivors than that leaves
// the sieve off (the exact walk runs) and the next one gets room.
int ensure_sieve(hvws_ctx* c, uint64_t rx_len, sieve_bufs& b) {
    const uint64_t* h = c->h_sv.as<uint64_t>();
    // entries before HBM verification, and survivors, of the latest sieved
    // scan whose state has landed (pipelined steps run ahead of it)
    if (sieve_state_ready(c)) {
        const uint64_t pre = h[sizeof(dsieve) / 8 + 3], surv = h[sizeof(dsieve) / 8];
        const bool counted = surv <= pre && pre <= c->sv_cap;   // else it overflowed and never counted survivors
        c->sv_hint_pre = pre;
        c->sv_hint_surv = counted ? surv : 0;
        // A windowed chain that stopped well before the end (a walk hit its
        // frame cap, or traffic changed): the next 15 scans sieve every tile.
        const dsieve* d = c->h_sv.as<dsieve>();
        if (c->sv_win_len && d->active && (!d->use || d->pend + (4ull << 20) < c->sv_win_len)) c->sv_full_left = 15;
        c->sv_hint_win = c->sv_win_len != 0;
        c->sv_win_len = 0;
        // bytes per frame along the last chain: the window geometry's mean
        // (single_hint is read only when the frame table had to be sized by
        // an estimate, so it can belong to an older stream)
        if (d->active && d->use && d->npath) c->sv_mean = std::max<uint64_t>(1, d->pend / d->npath);
    }
    if (c->sv_full_left) {
        --c->sv_full_left;
        b.rt = b.wt = 1;
    } else {
        sieve_geometry(rx_len, c->sv_mean ? rx_len / c->sv_mean : c->single_hint, b.rt, b.wt);
    }
    // Counts of a windowed scan say nothing about a scan of every tile.
    const bool stale = b.rt == b.wt && c->sv_hint_win;
    const uint64_t seen = stale ? 0 : c->sv_hint_pre, seen_s = stale ? 0 : c->sv_hint_surv;
    // Capacity from the last sieved scan's entry count when there is one (the
    // chain steps and their scans run over the whole capacity), else one
    // entry per KiB of the batch.
    uint64_t cap = seen ? std::max<uint64_t>({1ull << 18, rx_len / 8192, seen + seen / 4 + 1024})
                        : std::max<uint64_t>(1ull << 20, rx_len / 1024);
    cap = std::min<uint64_t>(cap, 0xFFFFFFF0ull);
    c->sv_cap = cap;
    // chain arrays: from the last survivor count (the chain steps scale with it)
    // (no usable count -- none yet, or the last scan overflowed its entries and
    // never counted survivors -- means the full capacity)
    uint64_t capc = seen_s ? std::min<uint64_t>(cap, std::max<uint64_t>(1ull << 16, seen_s + seen_s / 4 + 1024))
                           : cap;
    uint64_t scr_bytes = 0;
    b.lgP = 0;
    if (b.rt != b.wt && seen_s) {
        // Windowed: survivors lie in the windows only (a count from a scan of
        // every tile scales by their share).  A small capacity keeps the
        // doubling rounds in one LDS-resident launch and the walks' offset
        // scratch (2^lgP per node, about twice the frames a region holds) small.
        const uint64_t est = c->sv_hint_win ? seen_s : seen_s * b.wt / b.rt * 2;
        capc = std::min<uint64_t>(cap, std::max<uint64_t>(4096, est + est / 2 + 2048));
        uint32_t lgP = 4;
        while (lgP < 12 && (1ull << lgP) < 2 * sieve_hops()) ++lgP;
        if ((capc << lgP) <= (1ull << 25)) {
            scr_bytes = (capc << lgP) * 8;
            b.lgP = lgP;
        }
    }
    c->sv_capc = capc;
    const uint64_t ntm = sieve_tiles_max(rx_len);
    const uint64_t nmax = std::max(cap, ntm);
    // Every sieve buffer with the bytes this scan needs of it (0: not used).
    // No room for one of them: the tables are released, the state and the
    // counters stay, and the caller walks instead.
    const struct { dbuf* b; uint64_t bytes; } need[] = {{&c->sv_scr, scr_bytes},        {&c->sv_state, sizeof(dsieve)},
                {&c->sv_tcount, ntm * 8},       {&c->sv_tbase, ntm * 8},
                {&c->sv_slot, sieve_slot_words(rx_len) * 4},
                {&c->sv_S, capc * 8},           {&c->sv_Spre, cap * 8},
                {&c->sv_pool, cap * 4},         {&c->sv_keep, cap * 8},
                {&c->sv_kbase, cap * 8},        {&c->sv_J0, capc * 4},
                {&c->sv_J1, capc * 4},          {&c->sv_mark, capc * 8},
                {&c->sv_hops, capc * 4},        {&c->sv_rank, capc * 8},
                {&c->sv_cnt, 32},               {&c->sv_tmp, (4 * ((nmax + 1023) / 1024) + 64) * 8}};
    for (const auto& n : need) {
        if (!n.bytes || n.b->ensure(n.bytes) == hipSuccess) continue;
        (void)hipGetLastError();
        for (const auto& r : need)
            if (r.b != &c->sv_state && r.b != &c->sv_cnt) r.b->release();
        return set_err(HVWS_ENOMEM, "no room for the sieve's tables");
    }
    b.scr = scr_bytes ? c->sv_scr.as<uint64_t>() : nullptr;
    b.state = c->sv_state.as<dsieve>();
    b.tcount = c->sv_tcount.as<uint64_t>();
    b.tbase = c->sv_tbase.as<uint64_t>();
    b.slot = c->sv_slot.as<uint32_t>();
    b.pool = c->sv_pool.as<uint32_t>();
    b.pool_n = c->sv_cnt.as<uint64_t>() + 2;
    b.S = c->sv_S.as<uint64_t>();
    b.Spre = c->sv_Spre.as<uint64_t>();
    b.m_pre = c->sv_cnt.as<uint64_t>() + 3;
    b.J0 = c->sv_J0.as<uint32_t>();
    b.J1 = c->sv_J1.as<uint32_t>();
    b.mark = c->sv_mark.as<uint64_t>();
    b.hops = c->sv_hops.as<uint32_t>();
    b.rank = c->sv_rank.as<uint64_t>();
    b.m_total = c->sv_cnt.as<uint64_t>();
    b.npath = c->sv_cnt.as<uint64_t>() + 1;
    b.tmp = c->sv_tmp.as<uint64_t>();
    b.capS = cap;
    b.capC = capc;
    b.keep = c->sv_keep.as<uint64_t>();
    b.kbase = c->sv_kbase.as<uint64_t>();
    c->sv_win_len = b.rt != b.wt ? rx_len : 0;
    c->sv_rt = b.rt;
    c->sv_wt = b.wt;
    return HVWS_OK;
}

// Unmask kernel launch with its timing events (no argument checks).  The
// events ride on the unmask's own dispatch (launch_unmask).
// joined = true: the host has already seen the scan's last kernel publish
// (wait_status on tseq), so no cross-stream wait is queued before the unmask.
hipError_t issue_unmask(hvws_ctx* c, uint8_t* d_rx, uint64_t rx_len, bool joined = false) {
    hipError_t e;
    const bool piped = c->cs != c->stream;
    if (piped && !joined) {   // the scan ran on the side stream: join it
        if ((e = hipEventRecord(c->scan_done, c->cs)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(c->stream, c->scan_done, 0)) != hipSuccess) return e;
    }
    const bool timed = step_events(c) >= 1 && c->t_on;
    // Pipelined steps of mixed multi-segment batches: the unmask in pieces.
    // The hardware dispatches a kernel queued on the second stream (the next
    // batch's discovery) only once the unmask grid is fully launched, so its
    // walk (~0.2 ms at c4) waited for the whole unmask; between pieces it is
    // dispatched and overlaps.  On-device sweep: 4 pieces c4
    // 1.73 -> 1.55 ms, but c3 21.3 -> 22.4 ms and c2 flat, so uniform batches
    // (SPEC: a short scan) keep one launch.  With the 512 x 2 linear geometry
    // (round 2, profiles/r2n_raw) c4 ran 1.429 / 1.405 / 1.377 / 1.366 ms at
    // 1 / 2 / 4 / 8 pieces: 8.  One sieved stream (c4 as one segment, its
    // ~25 chain kernels beside the unmask) likewise: 1 / 2 / 4 / 8 / 12 / 16 /
    // 32 pieces 1.58 / 1.56 / 1.54 / 1.52 / 1.525 / 1.535 / 1.59 ms
    // (profiles/r5_raw/pieces).  $HVWS_EXPERIMENT unmask_pieces overrides.
    static const int env_pieces = experiment("unmask_pieces") ? atoi(experiment("unmask_pieces")) : -1;
    const int path = c->prev_path;   // the current scan's path may not be settled yet
    const bool mixed = path == HVWS_PATH_SLACK || path == HVWS_PATH_SLACK_FAILED || path == HVWS_PATH_SPEC_FAILED ||
                       (path == HVWS_PATH_COUNT_READ_EMIT && !c->spec_ok) ||   // an exact scan that saw mixed counts
                       (path == HVWS_PATH_SINGLE && c->sv_ran);                 // a sieved stream
    const uint32_t pieces = !piped ? 1u : env_pieces > 0 ? (uint32_t)env_pieces : (mixed ? 8u : 1u);
    // An untimed pipelined step attaches its set's free event to its last
    // dispatch (RUN: the repair) instead of recording it in a marker packet after it:
    // c2 0.355-0.356 vs 0.358 ms per step (profiles/r5_raw/events, fa*).
    const hipEvent_t ev_start = timed ? c->tev[c->t_cur][2] : nullptr;
    const hipEvent_t ev_stop = timed ? c->tev[c->t_cur][3] : (piped ? c->T().free_ev : nullptr);
    if (c->run_active)   // the RUN unmask and its repair pass (the stop event rides on the repair)
        e = launch_unmask_run(d_rx, rx_len, c->T().runs.as<drun>(), c->T().run_trun.as<dtrun>(), c->nseg,
                              c->T().run_fail.as<uint32_t>(), mapped<dspec_status>(c->h_status), c->run_seq, c->stream,
                              ev_start, ev_stop);
    else
        e = launch_unmask(c->variant, d_rx, rx_len, frames_of(c), c->T().tile_first.as<uint32_t>(),
                          c->T().tile_key.as<uint32_t>(), c->T().tile_kind.as<uint8_t>(), c->T().total.as<uint64_t>(),
                          c->stream, pieces, ev_start, ev_stop);
    if (e != hipSuccess) return e;
    if (timed) c->t_rec[c->t_cur] |= (uint8_t)(4u | 8u);
    c->t_unmask[c->t_cur] = true;
    if (piped) {   // the next pipelined scan into this set waits for this unmask
        // The unmask's dispatch-attached stop event marks the set free when it
        // was recorded; a separate marker packet cost ~6 us of device time per
        // pipelined c2 step (0.4215 -> 0.416 ms, profiles/r2r_raw).
        c->T().free_wait = timed ? c->tev[c->t_cur][3] : c->T().free_ev;
        c->T().free_pending = true;
    }
    return hipSuccess;
}

// One scan's inputs and working state, handed to the per-path functions below.
struct scan_job {
    hvws_ctx* c;
    const uint8_t* d_rx;
    uint64_t rx_len;
    uint32_t nseg;
    // The caller will unmask d_rx right after the scan (a step).  On the
    // checked paths the unmask is then queued before the host waits for the
    // device's check -- a rejected table has a zero count, so that unmask
    // does nothing -- and `unmasked` reports whether it stands.
    uint8_t* unmask_into;
    scan_scratch sc;
    dspec_status* status_d = nullptr;         // the pinned status, device-mapped
    const dspec_status* status_h = nullptr;   // ... and as the host reads it
    int up_slot = -1;                // upload slot the first pass frees (-1: none, or freed)
    uint64_t tile = 0, ntiles = 0;   // k_unmask geometry of the batch
    uint64_t bound = 0;              // record bound of the batch
    uint64_t nfr = 0;                // its records: the bound until a count has been read
    bool tiles_done = false;         // the tile kernels are queued
    bool unmasked = false;
};

// The current table set's scratch arrays and the upload the first pass reads.
scan_scratch scratch_of(hvws_ctx* c) {
    scan_scratch sc;
    sc.mid = c->T().sc_mid.as<dmid>();
    sc.npred = c->T().sc_npred.as<uint64_t>();
    sc.pbase = c->T().sc_pbase.as<uint64_t>();
    sc.first_fail = c->T().sc_fail.as<uint64_t>();
    sc.last_masked = c->T().sc_masked.as<uint64_t>();
    sc.total_pred = c->T().sc_total.as<uint64_t>();
    sc.est = c->T().sc_est.as<uint64_t>();
    sc.src_segs = c->up_src_segs;
    sc.src_carry = c->up_src_carry;
    sc.segs_w = c->segs.as<dseg>();
    sc.carry_w = c->carry_in.as<dcarry>();
    return sc;
}

// One pass of launch_scan.  After the first the device tables hold the
// uploaded segments; the pinned slot is free once its first kernel has run.
hipError_t issue_pass(scan_job& j, int which) {
    hvws_ctx* c = j.c;
    hipError_t e = launch_scan(which, j.d_rx, j.rx_len, c->segs.as<dseg>(), j.nseg, c->carry_in.as<dcarry>(),
                               c->T().carry_out.as<dcarry>(), c->T().counts.as<uint64_t>(), c->T().bases.as<uint64_t>(),
                               c->T().total.as<uint64_t>(), j.sc, frames_of(c), c->vmask, c->cs);
    j.sc.src_segs = nullptr;
    j.sc.src_carry = nullptr;
    if (e != hipSuccess || j.up_slot < 0) return e;
    e = hipEventRecord(c->up_ev[j.up_slot], c->cs);
    c->up_pending[j.up_slot] = e == hipSuccess;
    j.up_slot = -1;
    return e;
}

// The device's verdict for the pass just issued (after a wait on the stream
// or for the published status): the record count into j.nfr, the SPEC_* flags.
int read_status(scan_job& j, uint32_t& flags) {
    const dspec_status* st = j.status_h;
    if (st->seq != j.sc.seq) return set_err(HVWS_EHIP, "scan status not published (seq %llu, want %llu)",
                                            (unsigned long long)st->seq, (unsigned long long)j.sc.seq);
    j.nfr = st->total;
    flags = st->flags;
    if (flags & SPEC_ERR) return set_err(HVWS_EHIP, "scan check reported an error (seq %llu)",
                                         (unsigned long long)j.sc.seq);
    if (j.nfr >= 0xFFFFFFF0ull)
        return set_err(HVWS_EINVAL, "batch holds %llu frames (max 2^32-16)", (unsigned long long)j.nfr);
    return HVWS_OK;
}

// A rejected check in pipelined mode.  The speculative unmask was queued
// on c->stream, behind the previous batch's unmask, and reads this set's
// tile index and count when it runs, not when it was queued.  The exact
// re-scan rewrites those tables on c->cs; unordered, a still-waiting
// speculative unmask would see the re-scan's tiles and XOR for real, and
// the caller's unmask would then XOR the payloads back.  So the re-scan
// waits for it (the set's free event, recorded right after it).
int join_rejected(const scan_job& j) {
    hvws_ctx* c = j.c;
    if (j.unmask_into && c->cs != c->stream) HIP_OR(hipStreamWaitEvent(c->cs, c->T().free_wait, 0), HVWS_EHIP);
    return HVWS_OK;
}

int queue_tiles(const scan_job& j) {
    hvws_ctx* c = j.c;
    HIP_OR(launch_unmask_tiles(c->T().f_off.as<uint64_t>(), c->T().f_len.as<uint64_t>(), c->T().f_keyrot.as<uint32_t>(),
                               c->T().total.as<uint64_t>(), c->T().tile_first.as<uint32_t>(),
                               c->T().tile_key.as<uint32_t>(), c->T().tile_kind.as<uint8_t>(), j.ntiles, j.tile, j.rx_len,
                               c->cs),
           HVWS_EHIP);
    return HVWS_OK;
}

// One checked attempt: a pass whose table the device checks, with the tile
// kernels and the step's unmask queued before the host waits for the verdict,
// so the device runs on instead of idling through a host round trip.
// `which` is SCAN_SPEC, SCAN_SLACK, or SCAN_SINGLE for the capacity check of
// a one-segment pass that is already queued.  Accepted: j.tiles_done (and
// j.unmasked for a step).  Rejected: the count is zero on the device, so what
// was queued does nothing, and the re-scan is ordered behind it (join_rejected).
int checked_attempt(scan_job& j, int which, uint32_t& flags) {
    hvws_ctx* c = j.c;
    int rc;
    j.sc.seq = ++c->scan_seq;
    if (which == SCAN_SINGLE) {
        HIP_OR(launch_cap_check(c->T().total.as<uint64_t>(), c->T().frame_cap, j.status_d, j.sc.seq, c->cs), HVWS_EHIP);
    } else {
        // a set not used yet gets the other set's capacity (the table must
        // hold the batch for the check to pass: the last count, with room)
        const uint64_t other = c->ts[c->cur ^ 1].frame_cap;
        if (c->T().frame_cap < other) HIP_OR(ensure_frames(c, other, /*exact=*/true), HVWS_ENOMEM);
        j.sc.no_verify = (c->verify_mode < 0 ? c->verify_hint : c->verify_mode != 0) ? 0u : 1u;
        HIP_OR(issue_pass(j, which), HVWS_EHIP);
    }
    if ((rc = queue_tiles(j)) != HVWS_OK) return rc;
    // Pipelined SPEC: the host waits for the scan's last kernel (it runs
    // beside the previous unmask) and then queues this unmask with no
    // cross-stream wait packet between the two unmasks.  Otherwise the
    // unmask is queued behind the check at once.
    const bool ordered = which == SCAN_SPEC && j.unmask_into && c->cs != c->stream;
    if (ordered) {
        HIP_OR(launch_publish_tiles(j.status_d, j.sc.seq, c->cs), HVWS_EHIP);
    } else if (j.unmask_into) {
        HIP_OR(tev_record(c, 1, c->cs), HVWS_EHIP);
        HIP_OR(issue_unmask(c, j.unmask_into, j.rx_len), HVWS_EHIP);
    }
    if ((rc = wait_status(c, j.sc.seq)) != HVWS_OK) return rc;
    if ((rc = read_status(j, flags)) != HVWS_OK) return rc;
    const bool ok = (flags & SPEC_OK) != 0;
    if (which != SCAN_SINGLE) c->verify_hint = j.status_h->long_run_seen != 0;
    if (which == SCAN_SPEC) c->spec_ok = ok;   // before the unmask below: issue_unmask picks its pieces by it
    if (!ok) return join_rejected(j);
    if (ordered) {
        if ((rc = wait_status(c, j.sc.seq, /*tiles=*/true)) != HVWS_OK) return rc;
        HIP_OR(issue_unmask(c, j.unmask_into, j.rx_len, /*joined=*/true), HVWS_EHIP);
    }
    j.tiles_done = true;
    j.unmasked = j.unmask_into != nullptr;
    return HVWS_OK;
}

// A long one-segment batch is sieved (parallel discovery) unless the last
// sieved scan found uniform sizes: then 15 scans walk before the next try.
// Sets j.sc.sieve = &svb when this scan sieves.  Results never depend on it.
int choose_sieve(scan_job& j, sieve_bufs& svb) {
    hvws_ctx* c = j.c;
    if (c->sv_gen != sieve_generation()) {
        c->sv_gen = sieve_generation();
        c->sv_skip = 0;
        c->sv_ran = false;
        c->sv_hint_pre = c->sv_hint_surv = 0;
        c->sv_win_len = 0;
        c->sv_full_left = 0;
        c->sv_hint_win = false;
        c->sv_mean = 0;
    }
    if (j.rx_len < sieve_min()) return HVWS_OK;
    if (sieve_state_ready(c) && c->h_sv.as<dsieve>()->active == 0 && c->sv_skip == 0) c->sv_skip = 15;
    if (c->sv_skip) {
        --c->sv_skip;
        c->sv_ran = false;
        return HVWS_OK;
    }
    HIP_OR(c->h_sv.ensure(sizeof(dsieve) + 32), HVWS_ENOMEM);
    if (!c->sv_ev) HIP_OR(hipEventCreateWithFlags(&c->sv_ev, hipEventDisableTiming), HVWS_EHIP);
    // no room for the sieve's tables (ensure_sieve released them): walk instead
    c->sv_ran = ensure_sieve(c, j.rx_len, svb) == HVWS_OK;
    if (c->sv_ran) j.sc.sieve = &svb;
    return HVWS_OK;
}

// One stream: its base is 0, so EMIT needs no COUNT walk (a mixed-size
// stream's serial walk runs once).  The table is sized by the bound when that
// is small, else by an estimate (1.25 x the last one-stream count, at least
// 2^20 records) that is checked after the pass and re-emitted into an
// exact-size table if it overflowed.  (Sizing by the bound would give a
// 256 MiB chunk of 64 KiB frames a 3.2 GB table for its ~4000 records.)
int scan_single(scan_job& j) {
    hvws_ctx* c = j.c;
    int rc;
    c->scan_path = HVWS_PATH_SINGLE;
    const uint64_t guess = std::max<uint64_t>(kSingleMin, c->single_hint + c->single_hint / 4);
    HIP_OR(ensure_frames(c, std::min<uint64_t>(j.bound, guess)), HVWS_ENOMEM);
    sieve_bufs svb;
    if ((rc = choose_sieve(j, svb)) != HVWS_OK) return rc;
    HIP_OR(issue_pass(j, SCAN_SINGLE), HVWS_EHIP);
    if (j.bound > c->T().frame_cap) {
        // The table was sized by an estimate: the device checks the count
        // against it (over capacity zeroes the count) and publishes it.
        uint32_t flags = 0;
        if ((rc = checked_attempt(j, SCAN_SINGLE, flags)) != HVWS_OK) return rc;
        if (!j.tiles_done) {   // overflowed: re-emit into an exact table (the caller unmasks)
            HIP_OR(ensure_frames(c, j.nfr + 1), HVWS_ENOMEM);
            HIP_OR(issue_pass(j, SCAN_EMIT), HVWS_EHIP);
            HIP_OR(launch_offsets(c->T().counts.as<uint64_t>(), c->T().bases.as<uint64_t>(), 1,
                                  c->T().total.as<uint64_t>(), c->cs),
                   HVWS_EHIP);
        }
        c->nfr_known = true;
        c->single_hint = j.nfr;
    }
    if (c->sv_ran) {   // state and counts for the next scan's choices and hvws_last_sieve
        HIP_OR(hipMemcpyAsync(c->h_sv.p, c->sv_state.p, sizeof(dsieve), hipMemcpyDeviceToHost, c->cs), HVWS_EHIP);
        HIP_OR(hipMemcpyAsync(c->h_sv.as<uint8_t>() + sizeof(dsieve), c->sv_cnt.p, 32, hipMemcpyDeviceToHost, c->cs),
               HVWS_EHIP);
        HIP_OR(hipEventRecord(c->sv_ev, c->cs), HVWS_EHIP);
    }
    j.sc.sieve = nullptr;
    return HVWS_OK;
}

// Frame records are bounded: after a segment's first record every frame
// spends >= 2 of its bytes.  When the bound fits the table, EMIT follows
// COUNT with no host round trip and the count stays on the device (the
// tile kernels and k_unmask read it there).
int scan_bounded(scan_job& j) {
    hvws_ctx* c = j.c;
    c->scan_path = HVWS_PATH_COUNT_EMIT;
    HIP_OR(issue_pass(j, SCAN_COUNT), HVWS_EHIP);
    HIP_OR(ensure_frames(c, j.bound), HVWS_ENOMEM);
    HIP_OR(issue_pass(j, SCAN_EMIT), HVWS_EHIP);
    return HVWS_OK;
}

// Large batch: does this one take the RUN path?  A step's batch of small
// uniform frames (the last exact or SPEC scan matched the uniform estimates):
// discovery is k_head alone, the unmask checks every header it loads
// (hvws_internal.h, drun).  Segments of RUN_MIN_SEG bytes or more on average:
// k_unmask_run takes two segments per tile and leaves any between to the repair.
bool run_chosen(scan_job& j) {
    hvws_ctx* c = j.c;
    // The last RUN verdict the device has published: a failed hypothesis
    // turns RUN off for the next 16 steps and the next scan exact.
    const uint64_t vseq = __atomic_load_n(&j.status_h->run_seq, __ATOMIC_ACQUIRE);
    if (vseq != c->run_seen) {
        c->run_seen = vseq;
        if (j.status_h->run_failed) {
            c->run_skip = 16;
            c->spec_ok = false;
        }
    }
    const bool run_auto = c->run_mode < 0 && c->spec_ok && c->spec_mode != 0 && !c->run_skip && c->last_mean &&
                          c->last_mean <= RUN_MAX_FRAME && j.rx_len / j.nseg >= RUN_MIN_SEG && run_env();
    if (c->run_skip && !c->materializing) --c->run_skip;
    return j.unmask_into && c->run_call && c->vmask == 0 && (run_auto || c->run_mode == 1);
}

// RUN: run descriptors and the tile-segment index, then the unmask at once.
// No frame table, no count (finish_scan skips what needs them).
int scan_run(scan_job& j) {
    hvws_ctx* c = j.c;
    c->scan_path = HVWS_PATH_RUN;
    HIP_OR(c->T().runs.ensure((uint64_t)j.nseg * sizeof(drun) + 64), HVWS_ENOMEM);
    HIP_OR(c->T().run_fail.ensure_zeroed((uint64_t)j.nseg * 4 + 64, c->cs), HVWS_ENOMEM);
    j.sc.run_tile = RUN_TILE;
    j.sc.run_ntiles = (j.rx_len + RUN_TILE - 1) / RUN_TILE;
    HIP_OR(c->T().run_trun.ensure((j.sc.run_ntiles + 1) * sizeof(dtrun)), HVWS_ENOMEM);
    j.sc.runs = c->T().runs.as<drun>();
    j.sc.run_fail = c->T().run_fail.as<uint32_t>();
    j.sc.run_trun = c->T().run_trun.as<dtrun>();
    HIP_OR(issue_pass(j, SCAN_RUN), HVWS_EHIP);
    c->run_seq = ++c->scan_seq;
    c->run_active = true;
    c->run_vmask = c->vmask;
    c->nseg = j.nseg;   // issue_unmask reads it
    if (c->cs != c->stream) {   // pipelined: host-ordered, as SPEC (checked_attempt)
        HIP_OR(launch_publish_tiles(j.status_d, c->run_seq, c->cs), HVWS_EHIP);
        if (int rc = wait_status(c, c->run_seq, /*tiles=*/true)) return rc;
        HIP_OR(issue_unmask(c, j.unmask_into, j.rx_len, /*joined=*/true), HVWS_EHIP);
    } else {
        HIP_OR(tev_record(c, 1, c->cs), HVWS_EHIP);
        HIP_OR(issue_unmask(c, j.unmask_into, j.rx_len), HVWS_EHIP);
    }
    j.unmasked = true;
    j.nfr = 0;
    return HVWS_OK;
}

// SLACK's scratch table for this batch, if SLACK is to be tried: cap_seg
// records per segment region (1.5 x the last exact scan's largest segment).
// A scratch table that cannot be had is no error: scan exactly instead.
bool slack_table_ready(const scan_job& j, uint64_t& cap_seg) {
    hvws_ctx* c = j.c;
    cap_seg = c->slack_seg + c->slack_seg / 2 + 16;
    const uint64_t want = std::min<uint64_t>((uint64_t)j.nseg * cap_seg, j.bound) + 1;
    if (c->spec_mode == 0 || c->spec_mode == 1 || !c->slack_seg || !(c->spec_mode == 2 || !c->spec_ok) ||
        want > kSlackMaxRecords)
        return false;
    if (want <= c->sl_cap) return true;
    const uint64_t n = want + want / 4;
    dbuf* const tab[] = {&c->sl_hdr, &c->sl_off, &c->sl_len, &c->sl_length,   // 8 bytes per record
                         &c->sl_key, &c->sl_keyrot, &c->sl_info};             // 4
    bool ok = true;
    for (int i = 0; i < 7; ++i) ok = ok && tab[i]->ensure(n * (i < 4 ? 8 : 4)) == hipSuccess;
    c->sl_cap = ok ? n : 0;
    if (!ok) {
        (void)hipGetLastError();
        for (dbuf* b : tab) b->release();
    }
    return ok;
}

dframes slack_frames(hvws_ctx* c) {
    return {c->sl_hdr.as<int64_t>(), c->sl_off.as<uint64_t>(), c->sl_len.as<uint64_t>(), c->sl_length.as<uint64_t>(),
            c->sl_key.as<uint32_t>(), c->sl_keyrot.as<uint32_t>(), c->sl_info.as<uint32_t>(), c->sl_cap};
}

// Large batch: the table is sized from a count.  With the estimates holding
// on the last batch, EMIT speculatively into the table as it is (SCAN_SPEC)
// and let the device check it -- one walk, no host round trip before EMIT.
// Mixed sizes: one EMIT walk into per-segment regions of a scratch table,
// checked and compacted on the device (SCAN_SLACK); its check also tells
// whether the uniform estimates held (SPEC next time).  Otherwise, or when
// the check fails: COUNT, read the count, EMIT.
int scan_large(scan_job& j) {
    hvws_ctx* c = j.c;
    int rc;
    uint32_t flags = 0;
    uint64_t cap_seg;
    j.sc.status = j.status_d;
    c->scan_path = HVWS_PATH_COUNT_READ_EMIT;
    if ((c->spec_ok && c->spec_mode != 0) || c->spec_mode == 1) {
        if ((rc = checked_attempt(j, SCAN_SPEC, flags)) != HVWS_OK) return rc;
        c->scan_path = j.tiles_done ? HVWS_PATH_SPEC : HVWS_PATH_SPEC_FAILED;
    }
    if (!j.tiles_done && slack_table_ready(j, cap_seg)) {
        HIP_OR(c->sl_bx.ensure((uint64_t)j.nseg * 16 + 16), HVWS_ENOMEM);
        j.sc.slack = slack_frames(c);
        j.sc.slack_cap = cap_seg;
        j.sc.bases_x = c->sl_bx.as<uint64_t>();
        j.sc.est_u = c->sl_bx.as<uint64_t>() + j.nseg + 1;
        if ((rc = checked_attempt(j, SCAN_SLACK, flags)) != HVWS_OK) return rc;
        if (j.tiles_done) {
            c->slack_seg = j.status_h->max_seg_count;
            c->spec_ok = (flags & SPEC_MATCH) != 0;   // uniform again: the next batch tries SPEC
        }
        c->scan_path = j.tiles_done ? HVWS_PATH_SLACK : HVWS_PATH_SLACK_FAILED;
    }
    if (!j.tiles_done) {
        j.sc.seq = ++c->scan_seq;
        j.sc.no_verify = 0;
        HIP_OR(issue_pass(j, SCAN_COUNT), HVWS_EHIP);
        HIP_OR(hipStreamSynchronize(c->cs), HVWS_EHIP);
        if ((rc = read_status(j, flags)) != HVWS_OK) return rc;
        c->verify_hint = j.status_h->long_run_seen != 0;
        c->spec_ok = (flags & SPEC_MATCH) != 0;
        c->slack_seg = j.status_h->max_seg_count;
        HIP_OR(ensure_frames(c, j.nfr + 1), HVWS_ENOMEM);
        HIP_OR(issue_pass(j, SCAN_EMIT), HVWS_EHIP);
    }
    c->nfr_known = true;
    return HVWS_OK;
}

// Every path ends here.  A RUN scan left no frame table and has queued its
// unmask: no tile kernels, no scan-end event, no table check, no count.
int finish_scan(scan_job& j) {
    hvws_ctx* c = j.c;
    if (!c->run_active) {
        int rc;
        if (!j.tiles_done && (rc = queue_tiles(j)) != HVWS_OK) return rc;
        if (!j.unmasked) HIP_OR(tev_record(c, 1, c->cs), HVWS_EHIP);
        if (table_checks()) {   // the tile index's invariant (k_ends_check), tests only: one sync
            HIP_OR(c->chk.ensure(8), HVWS_ENOMEM);
            HIP_OR(c->h_chk.ensure(8), HVWS_ENOMEM);
            HIP_OR(hipMemsetAsync(c->chk.p, 0, 8, c->cs), HVWS_EHIP);
            HIP_OR(launch_ends_check(c->T().f_off.as<uint64_t>(), c->T().f_len.as<uint64_t>(),
                                     c->T().total.as<uint64_t>(), c->chk.as<unsigned long long>(), c->cs),
                   HVWS_EHIP);
            HIP_OR(hipMemcpyAsync(c->h_chk.p, c->chk.p, 8, hipMemcpyDeviceToHost, c->cs), HVWS_EHIP);
            HIP_OR(hipStreamSynchronize(c->cs), HVWS_EHIP);
            if (const uint64_t bad = *c->h_chk.as<uint64_t>())
                return set_err(HVWS_EINVAL, "frame table: %llu record ends before its predecessor's (scan path %d)",
                               (unsigned long long)bad, c->scan_path);
        }
    }
    c->nseg = j.nseg;
    c->nfr = j.nfr;
    c->rx = j.d_rx;
    c->rx_len = j.rx_len;
    c->have_scan = true;
    c->hcache_valid = false;
    if (c->nfr_known && j.nfr) c->last_mean = j.rx_len / j.nfr;
    return HVWS_OK;
}

// Discovery of one batch into the other table set: the preamble, the choice of
// path (one function each, above), finish_scan.  unmask_into, unmasked: scan_job.
int scan_device_carry(hvws_ctx* c, const uint8_t* d_rx, uint64_t rx_len, uint32_t nseg, uint8_t* unmask_into = nullptr,
                      bool* unmasked = nullptr) {
    if (unmasked) *unmasked = false;
    // The other table set: the previous batch's tables stay intact while its
    // unmask may still be running (pipelined steps).
    c->cur ^= 1;
    ++c->scan_gen;   // hvws_check: the passes before this scan ran over another table
    c->prev_path = c->scan_path;
    c->run_active = false;
    if (c->cs == c->stream) c->piped = false;   // a later pipelined step re-arms the set events
    if (c->cs != c->stream && c->T().free_pending) {
        HIP_OR(hipStreamWaitEvent(c->cs, c->T().free_wait, 0), HVWS_EHIP);
        c->T().free_pending = false;
    }
    tset& t = c->T();
    for (dbuf* b : {&t.counts, &t.bases, &t.sc_npred, &t.sc_pbase, &t.sc_fail, &t.sc_masked, &t.sc_est})
        HIP_OR(b->ensure((uint64_t)nseg * 8 + 8), HVWS_ENOMEM);   // one word per segment
    HIP_OR(t.total.ensure(8), HVWS_ENOMEM);
    HIP_OR(t.sc_total.ensure(8), HVWS_ENOMEM);
    HIP_OR(t.carry_out.ensure((uint64_t)nseg * sizeof(dcarry) + 64), HVWS_ENOMEM);
    HIP_OR(t.sc_mid.ensure((uint64_t)nseg * sizeof(dmid) + 64), HVWS_ENOMEM);
    HIP_OR(c->h_total.ensure(8), HVWS_ENOMEM);
    HIP_OR(c->h_status.ensure(sizeof(dspec_status)), HVWS_ENOMEM);
    HIP_OR(ensure_frames(c, 1), HVWS_ENOMEM);
    scan_job j{c, d_rx, rx_len, nseg, unmask_into, scratch_of(c)};
    j.status_d = mapped<dspec_status>(c->h_status);
    j.status_h = c->h_status.as<dspec_status>();
    if (!j.status_d) return set_err(HVWS_EHIP, "pinned status not device-mapped");
    // (run_materialize's rebuild of a RUN step's records keeps that step's
    // timing slot: no new slot, no events)
    if (!c->materializing) HIP_OR(begin_timed_scan(c), HVWS_EHIP);
    j.up_slot = c->up_slot;
    c->up_slot = -1;
    c->up_src_segs = nullptr;
    c->up_src_carry = nullptr;
    c->variant = unmask_variant_for(rx_len);
    j.tile = unmask_tile(c->variant);
    j.ntiles = (rx_len + j.tile - 1) / j.tile;
    HIP_OR(c->T().tile_first.ensure((j.ntiles + 8) * 4), HVWS_ENOMEM);
    HIP_OR(c->T().tile_key.ensure((j.ntiles + 2) * 4), HVWS_ENOMEM);
    HIP_OR(c->T().tile_kind.ensure(j.ntiles + 16), HVWS_ENOMEM);
    j.nfr = j.bound = rx_len / 2 + 2 * (uint64_t)nseg + 1;
    c->nfr_known = false;
    int rc;
    if (nseg == 1)
        rc = scan_single(j);
    else if (j.bound <= (c->fast_bound ? c->fast_bound : kFastFrameBound))
        rc = scan_bounded(j);
    else   // the table is sized from a count, or (RUN) not built at all
        rc = run_chosen(j) ? scan_run(j) : scan_large(j);
    if (rc == HVWS_OK) rc = finish_scan(j);
    if (unmasked) *unmasked = j.unmasked;
    return rc;
}

// The records of a RUN step, built when a reader asks for them: an exact scan
// of the same batch (its headers never change; its segment and carry tables
// are the device copies the RUN scan wrote) on the context stream, behind
// the unmask and its repair.  The scan path stays RUN, and the records are
// those of the validation classes in force when the step ran (none: a step
// under validation never takes the RUN path), whatever hvws_set_validation
// has been told since.
int run_materialize(hvws_ctx* c) {
    if (!c->run_active) return HVWS_OK;
    c->run_active = false;
    const int path = c->scan_path;
    hipStream_t cs = c->cs;
    c->cs = c->stream;
    const bool call = c->run_call, t_on = c->t_on;
    const uint32_t vmask = c->vmask;
    c->run_call = false;
    c->t_on = false;   // the RUN step's events stay in its slot (hvws_last_times / hvws_step_times)
    c->vmask = c->run_vmask;
    c->materializing = true;
    const int rc = scan_device_carry(c, c->rx, c->rx_len, c->nseg);
    c->materializing = false;
    c->vmask = vmask;
    c->t_on = t_on;
    c->run_call = call;
    c->cs = cs;
    c->scan_path = path;
    return rc;
}

// The frame count of the last scan on the host (one small read-back when the
// scan left it on the device).
int ensure_count(hvws_ctx* c) {
    if (int rc = run_materialize(c)) return rc;
    if (c->nfr_known) return HVWS_OK;
    HIP_OR(hipMemcpyAsync(c->h_total.p, c->T().total.p, 8, hipMemcpyDeviceToHost, c->stream), HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    c->nfr = *c->h_total.as<uint64_t>();
    c->nfr_known = true;
    return HVWS_OK;
}

// Everything a host-side replay needs from the last scan, in one round trip:
// count, per-segment first/count, carry-out, and the frame table up to the
// record bound (small batches) -- copied into pinned memory, one sync.
int readback_all(hvws_ctx* c) {
    if (int rc = run_materialize(c)) return rc;
    const uint32_t nseg = c->nseg;
    // c->nfr is the exact count or its bound; copy at most a prefix of the
    // table with the rest, and the remainder after the sync if needed.
    const uint64_t nrec = c->nfr < kReadbackPrefix ? c->nfr : kReadbackPrefix;
    const uint64_t cap = c->nfr_known ? c->nfr : nrec;
    const uint64_t soa = (cap > nrec ? cap : nrec) * (8 + 8 + 8 + 8 + 4 + 4);
    const uint64_t need = 64 + (uint64_t)nseg * (16 + sizeof(dcarry)) + soa + 64;
    HIP_OR(c->h_readback.ensure(need), HVWS_ENOMEM);
    uint8_t* h = c->h_readback.as<uint8_t>();
    uint64_t* total = (uint64_t*)h;
    uint64_t* first = (uint64_t*)(h + 64);
    uint64_t* count = first + nseg;
    dcarry* carry = (dcarry*)(count + nseg);
    hipStream_t s = c->stream;
    HIP_OR(hipMemcpyAsync(total, c->T().total.p, 8, hipMemcpyDeviceToHost, s), HVWS_EHIP);
    if (nseg) {
        HIP_OR(hipMemcpyAsync(first, c->T().bases.p, (uint64_t)nseg * 8, hipMemcpyDeviceToHost, s), HVWS_EHIP);
        HIP_OR(hipMemcpyAsync(count, c->T().counts.p, (uint64_t)nseg * 8, hipMemcpyDeviceToHost, s), HVWS_EHIP);
        HIP_OR(hipMemcpyAsync(carry, c->T().carry_out.p, (uint64_t)nseg * sizeof(dcarry), hipMemcpyDeviceToHost, s),
               HVWS_EHIP);
    }
    // SoA staging sized for `cap` records (exact count known) or the prefix
    uint64_t room = cap > nrec ? cap : nrec;
    uint8_t* f = (uint8_t*)(carry + nseg);
    int64_t* f_hdr = (int64_t*)f;
    uint64_t* f_off = (uint64_t*)(f_hdr + room);
    uint64_t* f_len = f_off + room;
    uint64_t* f_length = f_len + room;
    uint32_t* f_key = (uint32_t*)(f_length + room);
    uint32_t* f_info = f_key + room;
    auto copy_range = [&](uint64_t a, uint64_t b) -> hipError_t {
        if (b <= a) return hipSuccess;
        const uint64_t n = b - a;
        hipError_t e2;
        if ((e2 = hipMemcpyAsync(f_hdr + a, c->T().f_hdr.as<int64_t>() + a, n * 8, hipMemcpyDeviceToHost, s))) return e2;
        if ((e2 = hipMemcpyAsync(f_off + a, c->T().f_off.as<uint64_t>() + a, n * 8, hipMemcpyDeviceToHost, s))) return e2;
        if ((e2 = hipMemcpyAsync(f_len + a, c->T().f_len.as<uint64_t>() + a, n * 8, hipMemcpyDeviceToHost, s))) return e2;
        if ((e2 = hipMemcpyAsync(f_length + a, c->T().f_length.as<uint64_t>() + a, n * 8, hipMemcpyDeviceToHost, s)))
            return e2;
        if ((e2 = hipMemcpyAsync(f_key + a, c->T().f_key.as<uint32_t>() + a, n * 4, hipMemcpyDeviceToHost, s))) return e2;
        return hipMemcpyAsync(f_info + a, c->T().f_info.as<uint32_t>() + a, n * 4, hipMemcpyDeviceToHost, s);
    };
    HIP_OR(copy_range(0, c->nfr_known ? c->nfr : nrec), HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(s), HVWS_EHIP);
    const uint64_t got = c->nfr_known ? c->nfr : nrec;
    if (*total > got) {
        // more records than the speculative prefix: the exact count is known
        // now, so one more round trip copies the whole table
        c->nfr = *total;
        c->nfr_known = true;
        return readback_all(c);
    }
    const uint64_t n = *total;
    c->nfr = n;
    c->nfr_known = true;
    c->hcache.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
        hvws_frame& o = c->hcache[i];
        o.hdr_off = f_hdr[i];
        o.pay_off = f_off[i];
        o.pay_len = f_len[i];
        o.length = f_length[i];
        o.key = f_key[i];
        o.info = f_info[i];
    }
    c->hfirst.assign(first, first + nseg);
    c->hcount.assign(count, count + nseg);
    c->hcarry.assign(carry, carry + nseg);
    c->hcache_valid = true;
    return HVWS_OK;
}

int upload_segments(hvws_ctx* c, const hvws_segment* segs, const websocket_parser* carry, uint32_t nseg,
                    uint64_t rx_len) {
    for (uint32_t s = 0; s < nseg; ++s) {
        if (segs[s].off > rx_len || segs[s].len > rx_len - segs[s].off)
            return set_err(HVWS_EINVAL, "segment %u [%llu,+%llu) outside the %llu-byte buffer", s,
                           (unsigned long long)segs[s].off, (unsigned long long)segs[s].len,
                           (unsigned long long)rx_len);
        if (s && segs[s].off < segs[s - 1].off + segs[s - 1].len)
            return set_err(HVWS_EINVAL, "segments must be sorted and disjoint (segment %u)", s);
    }
    HIP_OR(c->segs.ensure((uint64_t)nseg * sizeof(dseg) + 64), HVWS_ENOMEM);
    HIP_OR(c->carry_in.ensure((uint64_t)nseg * sizeof(dcarry) + 64), HVWS_ENOMEM);
    // Pinned staging slot: the scan two uploads ago may still be about to
    // read it -- wait for that scan's first kernel only.
    const int u = c->up_next;
    c->up_next ^= 1;
    if (c->up_pending[u]) {
        HIP_OR(hipEventSynchronize(c->up_ev[u]), HVWS_EHIP);
        c->up_pending[u] = false;
    }
    const uint64_t o_carry = ((uint64_t)nseg * sizeof(dseg) + 63) & ~63ull;
    HIP_OR(c->h_up[u].ensure(o_carry + (uint64_t)nseg * sizeof(dcarry) + 64), HVWS_ENOMEM);
    dseg* hs = c->h_up[u].as<dseg>();
    dcarry* hc = reinterpret_cast<dcarry*>(c->h_up[u].as<uint8_t>() + o_carry);
    for (uint32_t s = 0; s < nseg; ++s) {
        hs[s].off = segs[s].off;
        hs[s].len = segs[s].len;
        if (carry) {
            to_dcarry(carry[s], hc[s]);
        } else {
            memset(&hc[s], 0, sizeof(dcarry));
        }
    }
    // No copy: the scan's first kernel reads the slot through its device
    // mapping and writes c->segs / c->carry_in (a DMA copy of these tables
    // cost ~40 us of idle device per step).
    uint8_t* dev = mapped<uint8_t>(c->h_up[u]);
    if (!dev) return set_err(HVWS_EHIP, "pinned upload slot not device-mapped");
    c->up_slot = u;
    c->up_src_segs = reinterpret_cast<const dseg*>(dev);
    c->up_src_carry = reinterpret_cast<const dcarry*>(dev + o_carry);
    return HVWS_OK;
}

// Device-visible address of pinned host memory (nullptr if `p` is not
// pinned/registered host memory).
uint8_t* host_mapped(void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer || !a.hostPointer) return nullptr;
    return (uint8_t*)a.devicePointer + ((uint8_t*)p - (uint8_t*)a.hostPointer);
}

bool small_eligible(hvws_ctx* c, uint64_t len, const hvws_segment* segs, uint32_t nseg) {
    const uint64_t limit = c->small_limit ? c->small_limit : kSmallBatch;
    if (c->small_limit == ~0ull || len > limit || nseg == 0) return false;
    for (uint32_t s = 0; s < nseg; ++s)
        if (segs[s].len > kSmallSegment) return false;
    return true;
}

// hvws_rx_batch for small batches: one H2D copy, k_small, one sync.
int rx_batch_small(hvws_ctx* c, uint8_t* h_rx, uint64_t len, const hvws_segment* segs, websocket_parser* carry,
                   uint32_t nseg, int unmask, uint8_t* dev_base = nullptr) {
    for (uint32_t s = 0; s < nseg; ++s) {
        if (segs[s].off > len || segs[s].len > len - segs[s].off)
            return set_err(HVWS_EINVAL, "segment %u [%llu,+%llu) outside the %llu-byte buffer", s,
                           (unsigned long long)segs[s].off, (unsigned long long)segs[s].len, (unsigned long long)len);
        if (s && segs[s].off < segs[s - 1].off + segs[s - 1].len)
            return set_err(HVWS_EINVAL, "segments must be sorted and disjoint (segment %u)", s);
    }
    // packet: [counter | segs | carry | slot_base | data (256-aligned)]
    const uint64_t o_segs = 64;
    const uint64_t o_carry = o_segs + (uint64_t)nseg * sizeof(dseg);
    const uint64_t o_slot = o_carry + (uint64_t)nseg * sizeof(dcarry);
    const uint64_t o_data = (o_slot + (uint64_t)nseg * 8 + 255) & ~255ull;
    // pinned caller buffer: read and write it directly.  dev_base (hvws_rx_reads):
    // the segments are the callers' registered pinned reads, offsets from dev_base.
    uint8_t* user_mapped = dev_base ? dev_base : host_mapped(h_rx);
    const uint64_t pkt = user_mapped ? o_data : o_data + len;
    // Segments of event-loop size are staged in LDS by k_small; small
    // batches of them may also go zero-copy (the kernel reads the packet and
    // the bytes from pinned host memory, no H2D copy ahead of the launch).
    uint64_t max_seg = 0;
    for (uint32_t s = 0; s < nseg; ++s) max_seg = std::max<uint64_t>(max_seg, segs[s].len);
    const bool stage = max_seg <= kStageSegment;
    const bool zc = dev_base || (stage && c->small_zc && len <= c->zc_batch);
    if (dev_base && !stage) return set_err(HVWS_EINVAL, "registered reads must be at most %llu bytes each",
                                           (unsigned long long)kStageSegment);
    const uint32_t stage_lds = stage ? (uint32_t)(((max_seg + 15) & ~15ull) + 16) : 0u;
    // The pinned packet may still be the source of an in-flight copy --
    // unless the last small call saw every completion word: then its copy
    // and its kernel's host accesses are over, and waiting for the stream
    // would only wait for the kernel's end-of-pipe signal (~10 us).
    if (!c->small_quiet) HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    c->small_quiet = false;
    // The packet carries the bytes only when the caller's buffer is not
    // device-mapped; the device copy exists only without zero-copy.  (With
    // dev_base, len spans all the reads' addresses, not bytes to move.)
    HIP_OR(c->h_small_in.ensure(o_data + (user_mapped ? 0 : len) + 64), HVWS_ENOMEM);
    if (!zc) HIP_OR(c->d_small_in.ensure(o_data + len + 64), HVWS_ENOMEM);
    uint8_t* hp = c->h_small_in.as<uint8_t>();
    memset(hp, 0, 64);
    dseg* hs = (dseg*)(hp + o_segs);
    dcarry* hc = (dcarry*)(hp + o_carry);
    uint64_t* hb = (uint64_t*)(hp + o_slot);
    uint64_t nslots = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
        hs[s].off = segs[s].off;
        hs[s].len = segs[s].len;
        if (carry) to_dcarry(carry[s], hc[s]);
        else memset(&hc[s], 0, sizeof(dcarry));
        hb[s] = nslots;
        nslots += segs[s].len / 2 + 3;   // carried-in frame + >= 2 bytes per frame + tail
    }
    if (!user_mapped && len) par_memcpy(hp + o_data, h_rx, len);
    const uint64_t hcap = std::min<uint64_t>(nslots, kSmallHostRecords);
    HIP_OR(c->d_small_slots.ensure(nslots * sizeof(drec) + 64), HVWS_ENOMEM);
    HIP_OR(c->h_small_out.ensure((uint64_t)nseg * sizeof(dsmall_out) + hcap * sizeof(drec) + 64), HVWS_ENOMEM);
    dsmall_out* ho = c->h_small_out.as<dsmall_out>();
    drec* hr = (drec*)(ho + nseg);
    dsmall_out* ho_d = mapped<dsmall_out>(c->h_small_out);
    uint8_t* hp_d = mapped<uint8_t>(c->h_small_in);
    if (!ho_d || !hp_d) return set_err(HVWS_EHIP, "pinned buffers not device-mapped");
    // Record counter: device memory, only ever grows; this call's records
    // start at small_ctr_base (no per-call reset operation).
    HIP_OR(c->d_small_ctr.ensure(64), HVWS_ENOMEM);
    unsigned long long* ctr = c->d_small_ctr.as<unsigned long long>();
    if (c->small_ctr_dirty) {
        HIP_OR(hipMemsetAsync(ctr, 0, 8, c->stream), HVWS_EHIP);
        c->small_ctr_base = 0;
        c->small_ctr_dirty = false;
    }
    const uint64_t ctr_base = c->small_ctr_base;
    c->small_ctr_dirty = true;   // until this call's record total is known
    uint8_t* d = hp_d;           // zero-copy: the kernel reads the pinned packet in place
    if (!zc) {
        d = c->d_small_in.as<uint8_t>();
        HIP_OR(hipMemcpyAsync(d, hp, pkt, hipMemcpyHostToDevice, c->stream), HVWS_EHIP);
        if (user_mapped && len)
            HIP_OR(hipMemcpyAsync(d + o_data, h_rx, len, hipMemcpyHostToDevice, c->stream), HVWS_EHIP);
    }
    const uint8_t* d_rx = zc ? (user_mapped ? user_mapped : hp_d + o_data) : d + o_data;
    // No timing events unless $HVWS_EXPERIMENT step_events >= 2 asks for them: an
    // event-carrying launch costs a per-read call ~10 us of ~38 (r2an).
    static const bool timed_env = experiment("step_events") && atoi(experiment("step_events")) >= 2;
    const bool timed = timed_env && c->t_on;
    // Completion: each wave releases its stores to system scope and then
    // writes its segment's word with this call's sequence number; the host
    // polls the words (in segment order) instead of waiting for the stream,
    // which also waits for the kernel's end-of-pipe release and signal.
    uint64_t* done_d = nullptr;
    const volatile uint64_t* done_h = nullptr;
    const uint64_t seq = ++c->small_seq;
    if (c->small_poll) {
        HIP_OR(c->h_small_done.ensure((uint64_t)nseg * 8 + 64), HVWS_ENOMEM);
        done_d = mapped<uint64_t>(c->h_small_done);
        done_h = c->h_small_done.as<uint64_t>();
        if (!done_d) return set_err(HVWS_EHIP, "pinned completion words not device-mapped");
    }
    HIP_OR(begin_timed_scan(c, false), HVWS_EHIP);
    HIP_OR(launch_small(d_rx, len, (const dseg*)(d + o_segs), (const dcarry*)(d + o_carry), nseg,
                        (const uint64_t*)(d + o_slot), c->d_small_slots.as<drec>(), ctr, ctr_base,
                        (drec*)(ho_d + nseg), hcap, ho_d, user_mapped ? user_mapped : hp_d + o_data, unmask,
                        c->vmask, stage_lds, done_d, seq, c->stream, timed ? c->tev[c->t_cur][0] : nullptr,
                        timed ? c->tev[c->t_cur][1] : nullptr),
           HVWS_EHIP);
    if (timed) c->t_rec[c->t_cur] |= 3u;
    if (done_h) {
        // Spin on the words; now and then ask the stream, so a kernel that
        // faulted (or was never dispatched) ends the wait with its error.
        // (The stream is asked at most every ~100 us: a query takes the
        // runtime's locks, and right after a launch one cost ~7 us.)
        uint32_t s = 0, spins = 0;
        auto next_query = std::chrono::steady_clock::now() + std::chrono::microseconds(100);
        while (s < nseg) {
            if (done_h[s] == seq) {
                ++s;
                continue;
            }
            if ((++spins & 63u) == 0 && std::chrono::steady_clock::now() >= next_query) {
                next_query = std::chrono::steady_clock::now() + std::chrono::microseconds(100);
                const hipError_t q = hipStreamQuery(c->stream);
                if (q == hipSuccess) {   // finished: every word is written
                    if (done_h[s] != seq) return set_err(HVWS_EHIP, "k_small finished without completing segment %u", s);
                    continue;
                }
                if (q != hipErrorNotReady) return set_err(HVWS_EHIP, "k_small: %s", hipGetErrorString(q));
            }
            __builtin_ia32_pause();
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    } else {
        HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    }
    c->small_quiet = true;
    if (!user_mapped && unmask && len) par_memcpy(h_rx, hp + o_data, len);
    // host cache in segment order
    uint64_t total = 0;
    for (uint32_t s = 0; s < nseg; ++s) total += ho[s].count;
    c->small_ctr_base = ctr_base + total;
    c->small_ctr_dirty = false;
    c->hcache.resize(total);
    c->hfirst.resize(nseg);
    c->hcount.resize(nseg);
    c->hcarry.resize(nseg);
    // A segment whose records fit the pinned area (first + count <= hcap)
    // wrote them there; the others left them in their device slots only.
    bool on_host = true;
    const drec* slots_base = c->d_small_slots.as<drec>();
    uint64_t k = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
        const uint64_t cnt = ho[s].count;
        c->hfirst[s] = k;
        c->hcount[s] = cnt;
        c->hcarry[s] = ho[s].st;
        if (cnt) {
            if (ho[s].first + cnt <= hcap) {
                memcpy(&c->hcache[k], hr + ho[s].first, cnt * sizeof(drec));
            } else {
                on_host = false;
                HIP_OR(hipMemcpyAsync(&c->hcache[k], slots_base + hb[s], cnt * sizeof(drec), hipMemcpyDeviceToHost,
                                      c->stream),
                       HVWS_EHIP);
            }
        }
        k += cnt;
    }
    if (!on_host) HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    c->nseg = nseg;
    c->nfr = total;
    c->nfr_known = true;
    c->rx = nullptr;   // the device frame table is not populated: hvws_unmask refuses
    c->rx_len = 0;
    ++c->scan_gen;
    c->have_scan = true;
    c->hcache_valid = true;
    if (carry) {
        for (uint32_t s = 0; s < nseg; ++s) {
            void* keep = carry[s].data;
            from_dcarry(c->hcarry[s], carry[s]);
            carry[s].data = keep;
        }
    }
    return HVWS_OK;
}

// ------------------------------------------------- resident small-path worker
// k_door (hvws_kernels.hip, ddoor in hvws_internal.h) serves the reference
// API's single calls -- FeedRecvData / websocket_parser_execute on one read,
// websocket_decode, websocket_parser_decode, a masked websocket_build_frame --
// from a mailbox in fine-grained pinned memory: no launch, no dispatch and no
// end-of-kernel signal per call.

// Idle time after which a worker parks ($HVWS_EXPERIMENT door_idle_us, default 5 ms),
// in ticks of the 100 MHz realtime clock.
std::atomic<uint64_t> g_door_idle_us{0};   // 0: not yet read from the environment

uint64_t door_idle_us() {
    uint64_t us = g_door_idle_us.load(std::memory_order_relaxed);
    if (!us) {
        const char* e = experiment("door_idle_us");
        us = e && strtoull(e, nullptr, 0) ? strtoull(e, nullptr, 0) : 5000;
        g_door_idle_us.store(us, std::memory_order_relaxed);
    }
    return us;
}

uint64_t door_idle_ticks() { return door_idle_us() * 100; }

bool door_on(hvws_ctx* c) {
    if (c->door_broken) return false;
    if (c->door_mode >= 0) return c->door_mode != 0;
    static const int env = getenv("HVWS_DOOR") ? atoi(getenv("HVWS_DOOR")) : 1;   // on by default (round 4)
    return env != 0;
}

// Contexts that own a worker queue.  Lock order: g_door_m, then a
// context's door_m; nothing that holds a door_m takes g_door_m.
std::mutex g_door_m;
std::vector<hvws_ctx*> g_doors;
// Idle worker queues of released contexts, for the next context's worker on
// that device (creating one is the costliest step of a context's first call);
// destroyed at exit.  Guarded by g_door_m.
std::vector<door_queue*> g_door_pool;
std::atomic<int> g_door_count{0};   // g_doors.size(): frees skip the lock when no worker exists
void door_atexit();
// Process-wide failure counts (hvws_door_health; the test session fails on
// either): worker streams that did not drain within their bound (left
// wedged), and requests a worker did not answer (the context then launches
// per call).  Both are printed to stderr as they happen.
std::atomic<uint64_t> g_door_wedged{0};
std::atomic<uint64_t> g_door_failed{0};

// Worker streams per device at most ($HVWS_DOOR_MAX, default 8): each is a
// hardware queue of its own, and queues beyond what the hardware scheduler
// maps at once are time-sliced -- a resident worker could then go
// unscheduled.  A context past the cap serves its reads with a launch each.
int door_cap() {
    static const int cap = getenv("HVWS_DOOR_MAX") && atoi(getenv("HVWS_DOOR_MAX")) > 0 ? atoi(getenv("HVWS_DOOR_MAX")) : 8;
    return cap;
}

// Marks the runtime call a context is in for the wedge report and
// hvws_debug_dump (a hang then names its call, not only its thread).
struct in_call {
    hvws_ctx* c;
    const char* prev;
    in_call(hvws_ctx* c_, const char* what) : c(c_), prev(c_->at.exchange(what)) {}
    ~in_call() { c->at.store(prev); }
};

// The request area in device memory: its 128-byte request block, then the
// request bytes.
constexpr uint64_t kDoorReqBytes = 256 + kDoorMax + 256;

bool door_vram_enabled() {
    static const int v = experiment("door_vram") ? atoi(experiment("door_vram")) : 1;
    return v != 0;
}

// Host stores to device memory go through write-combining buffers: an sfence
// makes them visible (the request bytes before seq, and seq itself; without
// it a lone 8-byte seq store sat in a WC buffer for ~10 ms,
// profiles/r4a_raw/vram_probe.jsonl).
inline void door_flush_wc() { __builtin_ia32_sfence(); }

// A request's bytes into the mailbox.  Device memory behind the BAR is
// write-combining: with AVX-512 every store is one whole 64-byte line, a
// non-temporal one (the sfence in door_call drains them); otherwise memcpy.
__attribute__((target("avx512f"))) void wc_copy_avx512(uint8_t* dst, const uint8_t* src, size_t n) {
    size_t i = 0;
    for (; i + 64 <= n; i += 64) _mm512_stream_si512((__m512i*)(dst + i), _mm512_loadu_si512(src + i));
    if (i < n) memcpy(dst + i, src + i, n - i);
}
void door_copy_in(hvws_ctx* c, uint8_t* dst, const void* src, size_t n) {
    static const bool avx512 = __builtin_cpu_supports("avx512f");
    if (c->d_door_req && avx512 && ((uintptr_t)dst & 63u) == 0) wc_copy_avx512(dst, static_cast<const uint8_t*>(src), n);
    else memcpy(dst, src, n);
}

// Where the host writes a request (block and bytes) and where the worker reads it.
ddoor* door_req(hvws_ctx* c) { return c->d_door_req ? (ddoor*)c->d_door_req : c->h_door.as<ddoor>(); }
uint8_t* door_din(hvws_ctx* c) {
    return c->d_door_req ? (uint8_t*)c->d_door_req + 256 : c->h_door_data.as<uint8_t>();
}

// A context that gets no worker serves its calls with a launch each (its
// callers fall back on any failure here), so the thread's last-error text is
// left as it was: the call itself succeeds.
int door_ensure_impl(hvws_ctx* c);
int door_ensure(hvws_ctx* c) {
    if (c->door_q) return HVWS_OK;
    char saved[sizeof g_err];
    memcpy(saved, g_err, sizeof g_err);
    const int rc = door_ensure_impl(c);
    if (rc != HVWS_OK) memcpy(g_err, saved, sizeof g_err);
    return rc;
}

int door_ensure_impl(hvws_ctx* c) {
    {
        std::lock_guard<std::mutex> lk(g_door_m);
        int same = 0;
        for (const hvws_ctx* o : g_doors) same += o->device == c->device;
        if (same >= door_cap()) return set_err(HVWS_EINVAL, "k_door: %d workers on device %d already", same, c->device);
    }
    HIP_OR(hipSetDevice(c->device), HVWS_EHIP);
    hipDeviceProp_t prop;
    HIP_OR(hipGetDeviceProperties(&prop, c->device), HVWS_EHIP);
    // The mailbox is fine-grained (polled, uncached); the data and record
    // areas are ordinary pinned memory: the worker's system-scope acquire on
    // each request invalidates its caches before it stages the bytes, and its
    // release writes its results back.  (Fine-grained data made the staging
    // loads of an 8 KiB read take 6.2 us, profiles/r3f_raw.)
    c->h_door.flags = hipHostMallocCoherent;
    HIP_OR(c->h_door.ensure(sizeof(ddoor)), HVWS_ENOMEM);
    HIP_OR(c->h_door_data.ensure(kDoorMax + 256), HVWS_ENOMEM);
    HIP_OR(c->h_door_rec.ensure(kDoorRecords * sizeof(drec)), HVWS_ENOMEM);
    HIP_OR(c->d_door_slot.ensure(kDoorRecords * sizeof(drec)), HVWS_ENOMEM);
    memset(c->h_door.p, 0, sizeof(ddoor));
    if (!mapped<ddoor>(c->h_door) || !mapped<uint8_t>(c->h_door_data) || !mapped<drec>(c->h_door_rec))
        return set_err(HVWS_EHIP, "worker mailbox not device-mapped");
    if (door_vram_enabled() && prop.isLargeBar && !c->d_door_req) {
        // With a large BAR, fine-grained device memory is mapped for the host
        // at its device address (profiles/r4a_raw/vram_probe.jsonl: host
        // stores and loads work, an 8 KiB memcpy into it takes 0.49 us);
        // without one the request area stays pinned host memory.
        void* p = nullptr;
        if (hipExtMallocWithFlags(&p, kDoorReqBytes, hipDeviceMallocFinegrained) == hipSuccess) {
            c->d_door_req = p;
            memset(p, 0, sizeof(ddoor));
            door_flush_wc();
        }
        (void)hipGetLastError();
    }
    std::lock_guard<std::mutex> lk(g_door_m);
    int same = 0;   // again, under the lock that also registers this context
    for (const hvws_ctx* o : g_doors) same += o->device == c->device;
    if (same >= door_cap()) return set_err(HVWS_EINVAL, "k_door: %d workers on device %d already", same, c->device);
    for (size_t i = 0; i < g_door_pool.size(); ++i)
        if (g_door_pool[i]->device == c->device) {
            c->door_q = g_door_pool[i];
            g_door_pool.erase(g_door_pool.begin() + (long)i);
            break;
        }
    if (!c->door_q) {
        in_call ic(c, "hsa_queue_create (worker queue)");
        if (int rc = door_queue_create(c->device, &c->door_q)) return set_err(rc, "%s", door_queue_why());
    }
    // registered after the HIP runtime's own exit handlers, so it runs before them
    static const bool reg = (atexit(door_atexit), true);
    (void)reg;
    g_doors.push_back(c);
    g_door_count.store((int)g_doors.size(), std::memory_order_release);
    return HVWS_OK;
}

uint64_t door_word(const hvws_ctx* c, const uint64_t& w) {
    (void)c;
    return __atomic_load_n(&w, __ATOMIC_ACQUIRE);
}

// Wait up to `ms` for the worker's last launch to end (its completion
// signal: never an unbounded wait -- a worker that never ends must not hang
// its host thread).  On a timeout the mailbox state goes to stderr and the
// context is marked wedged: its queue and mailbox are never reused or freed.
bool door_drain(hvws_ctx* c, int ms, const char* where) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        if (door_queue_idle(c->door_q)) return true;
        if (const int e = door_queue_error(c->door_q)) {
            set_err(HVWS_EHIP, "k_door: worker queue error 0x%x", e);
            return true;   // the queue failed: nothing of the worker runs any more
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(ms)) break;
        usleep(20);
    }
    const ddoor* b = c->h_door.as<ddoor>();
    const ddoor* rq = door_req(c);
    fprintf(stderr,
            "[hvws] k_door (%s): ctx %p worker launch still running after %d ms: seq %llu done %llu alive %llu "
            "exited %llu epoch %llu served %llu live %d\n",
            where, (void*)c, ms, (unsigned long long)__atomic_load_n(&rq->seq, __ATOMIC_ACQUIRE),
            (unsigned long long)door_word(c, b->done), (unsigned long long)door_word(c, b->alive),
            (unsigned long long)door_word(c, b->exited), (unsigned long long)c->door_epoch,
            (unsigned long long)door_word(c, b->served), (int)c->door_live);
    c->door_wedged = true;
    g_door_wedged.fetch_add(1);
    set_err(HVWS_EHIP, "k_door: the worker launch did not end (%s)", where);
    return false;
}

// Post the request already written into the mailbox and wait for it (the
// caller holds c->door_m).  A worker is (re)launched when none is resident.
// Whether the resident one has ended is read from the mailbox: its last
// store is `exited = epoch`; a relaunch also waits for the last launch's
// completion signal (door_drain), so two workers never share the mailbox.
// The queue's error state says whether a kernel fault ended it.
// pf, pf_len: results the caller copies out once `done` is seen.  The
// worker's stores land in host memory before `done` (its release waits for
// them), so prefetching those lines while waiting pulls them into the cache
// as they land instead of after `done`.
int door_call(hvws_ctx* c, const void* pf = nullptr, size_t pf_len = 0) {
    ddoor* b = c->h_door.as<ddoor>();
    ddoor* rq = door_req(c);
    const uint64_t seq = ++c->door_seq;
    rq->seq_tail = seq;
    if (c->d_door_req) door_flush_wc();   // the request's bytes and fields first
    __atomic_store_n(&rq->seq, seq, __ATOMIC_RELEASE);
    if (c->d_door_req) door_flush_wc();
    ++c->door_calls;
    const auto t0 = std::chrono::steady_clock::now();
    auto next_query = t0 + std::chrono::microseconds(100);
    uint32_t spins = 0, launches = 0;
    for (;;) {
        if (__atomic_load_n(&b->done, __ATOMIC_ACQUIRE) == seq) return HVWS_OK;
        if (!c->door_live) {
            if (c->door_wedged) return set_err(HVWS_EHIP, "k_door: the worker stream is wedged");
            if (launches++ >= 4) return set_err(HVWS_EHIP, "k_door: the worker takes no requests");
            HIP_OR(hipSetDevice(c->device), HVWS_EHIP);
            __atomic_store_n(&b->alive, 1ull, __ATOMIC_RELAXED);
            ++c->door_epoch;
            const ddoor* dreq = c->d_door_req ? (const ddoor*)c->d_door_req : mapped<ddoor>(c->h_door);
            const uint8_t* ddin = c->d_door_req ? (const uint8_t*)c->d_door_req + 256 : mapped<uint8_t>(c->h_door_data);
            door_args a;
            a.req = dreq;
            a.box = mapped<ddoor>(c->h_door);
            a.din = ddin;
            a.dout = mapped<uint8_t>(c->h_door_data);
            a.h_rec = mapped<drec>(c->h_door_rec);
            a.d_slot = c->d_door_slot.as<drec>();
            a.idle_ticks = door_idle_ticks();
            a.first_seq = __atomic_load_n(&b->done, __ATOMIC_ACQUIRE);
            a.epoch = c->door_epoch;
            a.flags = door_flags();
            in_call ic(c, "AQL dispatch of k_door (worker queue)");
            if (int rc = door_queue_launch(c->door_q, &a, (uint32_t)sizeof a)) return set_err(rc, "%s", door_queue_why());
            c->door_live = true;
            ++c->door_launches;
            continue;
        }
        if (door_word(c, b->exited) == c->door_epoch) {
            // The worker has ended; its last look at seq came before this
            // request.  Its launch completes (the wave retires) before the
            // next launch, so two workers never share the mailbox.
            if (__atomic_load_n(&b->done, __ATOMIC_ACQUIRE) == seq) return HVWS_OK;
            if (!door_drain(c, 5000, "relaunch")) return HVWS_EHIP;
            c->door_live = false;
            continue;
        }
        if ((++spins & 63u) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (now >= next_query) {
                next_query = now + std::chrono::microseconds(100);
                if (const int e = door_queue_error(c->door_q)) return set_err(HVWS_EHIP, "k_door: worker queue error 0x%x", e);
                if (now - t0 > std::chrono::seconds(10)) return set_err(HVWS_EHIP, "k_door: no answer in 10 s");
            }
        }
        if (pf_len)
            for (size_t i = 0; i < pf_len; i += 64) __builtin_prefetch(static_cast<const char*>(pf) + i);
        else
            __builtin_ia32_pause();
    }
}

// Send the resident worker home and wait until it has ended (the caller
// holds c->door_m): context teardown, a free, a thread's exit, the door
// switched off.
void door_park(hvws_ctx* c) {
    if (!c->door_q || !c->door_live || c->door_wedged) return;
    ddoor* b = c->h_door.as<ddoor>();
    if (door_word(c, b->exited) != c->door_epoch) {
        door_req(c)->op = DOOR_EXIT;
        if (door_call(c) != HVWS_OK) {
            (void)hipGetLastError();
        } else {
            // served: the worker's `exited` store follows `done`
            const auto t0 = std::chrono::steady_clock::now();
            while (door_word(c, b->exited) != c->door_epoch &&
                   std::chrono::steady_clock::now() - t0 < std::chrono::seconds(1))
                __builtin_ia32_pause();
        }
    }
    if (door_drain(c, 5000, "park")) c->door_live = false;
}

// The calling thread's context for the reference-API entry points.
thread_local int t_device = -1;
thread_local hvws_ctx* t_ctx = nullptr;

// Park every worker on the current device before a free (whichever thread
// owns it); the current device is restored afterwards.
void door_park_device() {
    if (g_door_count.load(std::memory_order_acquire) == 0) return;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return;
    std::lock_guard<std::mutex> lk(g_door_m);
    for (hvws_ctx* c : g_doors) {
        if (c->device != dev || !c->door_live) continue;
        std::lock_guard<std::mutex> cl(c->door_m);
        door_park(c);
    }
    hipSetDevice(dev);
}

// At process exit: no HIP call at all (an exit handler that destroyed the
// worker streams hung a process's exit, profiles/r3ab_raw).  A worker still
// resident is asked to exit through the mailbox and given up to 100 ms to
// say it has ended; a context whose owner holds its lock past 100 ms is left
// as it is.
void door_quit_nohip(hvws_ctx* c) {
    if (!c->door_q || !c->door_live) return;
    ddoor* b = c->h_door.as<ddoor>();
    if (door_word(c, b->exited) != c->door_epoch) {
        ddoor* rq = door_req(c);
        rq->op = DOOR_EXIT;
        rq->seq_tail = c->door_seq + 1;
        if (c->d_door_req) door_flush_wc();
        __atomic_store_n(&rq->seq, ++c->door_seq, __ATOMIC_RELEASE);
        if (c->d_door_req) door_flush_wc();
        const auto t0 = std::chrono::steady_clock::now();
        while (door_word(c, b->exited) != c->door_epoch &&
               std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(100))
            __builtin_ia32_pause();
    }
    c->door_live = false;
}

// At exit, once every worker has ended (its launch's completion signal),
// the worker queues are destroyed (HSA calls only; this handler runs before
// the HIP runtime's own, so the HSA runtime is still up).  A process that
// ended with a worker queue alive crashed under rocprofv3; a
// queue whose worker did not end is left alone.
void door_atexit() {
    std::lock_guard<std::mutex> lk(g_door_m);
    for (hvws_ctx* c : g_doors) {
        std::unique_lock<std::mutex> cl(c->door_m, std::defer_lock);
        const auto t0 = std::chrono::steady_clock::now();
        while (!cl.try_lock() && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(100)) usleep(100);
        if (!cl.owns_lock()) continue;
        door_quit_nohip(c);
        if (!c->door_q || c->door_wedged) continue;
        const auto t1 = std::chrono::steady_clock::now();
        while (!door_queue_idle(c->door_q) && std::chrono::steady_clock::now() - t1 < std::chrono::milliseconds(100))
            usleep(50);
        if (door_queue_idle(c->door_q)) {
            c->door_q->at_exit = true;
            door_queue_destroy(c->door_q);
            c->door_q = nullptr;
        }
    }
    for (door_queue* q : g_door_pool) {
        q->at_exit = true;
        door_queue_destroy(q);
    }
    g_door_pool.clear();
}

void door_release(hvws_ctx* c) {
    if (!c->door_q) return;
    {
        std::lock_guard<std::mutex> lk(g_door_m);
        {
            std::lock_guard<std::mutex> cl(c->door_m);
            door_park(c);
        }
        g_doors.erase(std::remove(g_doors.begin(), g_doors.end(), c), g_doors.end());
        g_door_count.store((int)g_doors.size(), std::memory_order_release);
    }
    if (c->door_wedged || !door_drain(c, 5000, "release")) {
        // a worker that may still run: its queue and the memory it writes stay
        fprintf(stderr, "[hvws] k_door: ctx %p released with its worker launch wedged; queue and mailbox leaked\n",
                (void*)c);
        c->door_q = nullptr;
        c->h_door.p = c->h_door_data.p = c->h_door_rec.p = nullptr;
        c->d_door_slot.p = nullptr;
        c->d_door_req = nullptr;
        return;
    }
    {
        // ended: the next context's worker takes the queue (destroyed at exit)
        std::lock_guard<std::mutex> lk(g_door_m);
        g_door_pool.push_back(c->door_q);
    }
    c->door_q = nullptr;
    in_call ic(c, "hipHostFree / hipFree (worker mailbox and areas)");
    c->h_door.release();
    c->h_door_data.release();
    c->h_door_rec.release();
    c->d_door_slot.release();
    if (c->d_door_req) {
        door_park_device();
        hipFree(c->d_door_req);
        c->d_door_req = nullptr;
    }
}

// A request the worker did not answer (the caller holds c->door_m): counted
// and reported, and the context launches per call from now on.  The caller's
// buffer is untouched until a request succeeds, so the caller serves this
// call on the launch path itself (advisor r4: no abort).
void door_fail(hvws_ctx* c, const char* what) {
    g_door_failed.fetch_add(1);
    fprintf(stderr, "[hvws] k_door: ctx %p: %s request unanswered (%s); this context launches per call from now on\n",
            (void*)c, what, g_err);
    c->door_broken = true;
    if (c->door_live && !c->door_wedged && door_drain(c, 1000, "failed request")) c->door_live = false;
}

// $HVWS_EXPERIMENT feed_times=1: host time per phase of door_feed (request
// written, answered, results copied back), printed at exit (diagnostic).
struct door_times {
    bool on = experiment("feed_times") && atoi(experiment("feed_times"));
    std::atomic<uint64_t> calls{0}, ns[3] = {};
    ~door_times() {
        const uint64_t n = calls.load();
        if (on && n)
            fprintf(stderr, "[door_times] calls=%llu us/call: request %.2f answer %.2f results %.2f\n",
                    (unsigned long long)n, ns[0].load() / 1e3 / n, ns[1].load() / 1e3 / n, ns[2].load() / 1e3 / n);
    }
};
door_times g_door_times;

// One read through the worker (gpu_feed's fast path): false when the worker
// does not take it (off, or longer than kDoorMax).
bool door_feed(hvws_ctx* c, char* buf, size_t len, const websocket_parser& carry, bool unmask,
               std::vector<hvws_frame>& frames, websocket_parser& carry_out, int& started) {
    if (!door_on(c) || len > kDoorMax || door_ensure(c) != HVWS_OK) return false;
    std::lock_guard<std::mutex> cl(c->door_m);
    using clk = std::chrono::steady_clock;
    const bool timed = g_door_times.on;
    clk::time_point t0, t1, t2;
    if (timed) t0 = clk::now();
    ddoor* b = c->h_door.as<ddoor>();
    ddoor* rq = door_req(c);
    uint8_t* data = c->h_door_data.as<uint8_t>();
    door_copy_in(c, door_din(c), buf, len);
    rq->op = DOOR_FEED;
    rq->unmask = unmask ? 1u : 0u;
    rq->len = len;
    rq->vmask = c->vmask;
    dcarry cin;
    to_dcarry(carry, cin);
    memcpy(&rq->carry, &cin, sizeof(dcarry));
    if (timed) t1 = clk::now();
    if (door_call(c, data, unmask ? len : 0) != HVWS_OK) {
        door_fail(c, "read");
        return false;
    }
    if (timed) t2 = clk::now();
    const uint64_t n = b->count;
    frames.resize((size_t)n);
    if (n) memcpy(frames.data(), c->h_door_rec.p, (size_t)n * sizeof(drec));
    if (unmask) memcpy(buf, data, len);
    copy_parser(carry_out, carry);
    const dcarry out = b->out;
    from_dcarry(out, carry_out);
    started = (int)out.started;
    if (timed) {
        const auto t3 = clk::now();
        g_door_times.calls.fetch_add(1, std::memory_order_relaxed);
        g_door_times.ns[0].fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count());
        g_door_times.ns[1].fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t1).count());
        g_door_times.ns[2].fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t3 - t2).count());
    }
    return true;
}

bool door_xor(hvws_ctx* c, char* dst, const char* src, size_t n, uint32_t key, uint32_t phase) {
    if (!door_on(c) || n > kDoorMax || door_ensure(c) != HVWS_OK) return false;
    std::lock_guard<std::mutex> cl(c->door_m);
    ddoor* rq = door_req(c);
    uint8_t* data = c->h_door_data.as<uint8_t>();
    door_copy_in(c, door_din(c), src, n);
    rq->op = DOOR_XOR;
    rq->len = n;
    rq->key = key;
    rq->phase = phase;
    if (door_call(c, data, n) != HVWS_OK) {
        door_fail(c, "XOR");
        return false;
    }
    memcpy(dst, data, n);
    return true;
}

// ------------------------------------------- registered pinned host memory
// Ranges the device can read and write in place (hvws_host_alloc,
// hvws_host_register).  hvws_rx_reads looks every read up here; a
// thread-local last hit makes the common case (many reads out of one pinned
// arena) one compare per read.
struct pinned_range {
    uintptr_t lo, hi;
    uint8_t* dev;
    bool registered;   // hipHostRegister'ed (unregister on removal), else hipHostMalloc'ed
};
std::shared_mutex g_pin_m;
std::vector<pinned_range> g_pins;     // sorted by lo, disjoint
std::atomic<uint64_t> g_pin_gen{1};   // bumped on every removal

void pin_add(void* p, uint64_t bytes, uint8_t* dev, bool registered) {
    std::unique_lock<std::shared_mutex> lk(g_pin_m);
    const pinned_range r{(uintptr_t)p, (uintptr_t)p + bytes, dev, registered};
    g_pins.insert(std::upper_bound(g_pins.begin(), g_pins.end(), r,
                                   [](const pinned_range& a, const pinned_range& b) { return a.lo < b.lo; }),
                  r);
}

// Removes the range starting at p; returns it (lo == 0 if none).
pinned_range pin_remove(void* p) {
    std::unique_lock<std::shared_mutex> lk(g_pin_m);
    for (auto it = g_pins.begin(); it != g_pins.end(); ++it)
        if (it->lo == (uintptr_t)p) {
            const pinned_range r = *it;
            g_pins.erase(it);
            g_pin_gen.fetch_add(1);
            return r;
        }
    return pinned_range{0, 0, nullptr, false};
}

// Device address of [p, p+len) if it lies inside one registered range.
uint8_t* pinned_dev(const void* p, uint64_t len) {
    thread_local pinned_range last{0, 0, nullptr, false};
    thread_local uint64_t last_gen = 0;
    const uintptr_t a = (uintptr_t)p;
    const uint64_t gen = g_pin_gen.load(std::memory_order_acquire);
    if (last_gen != gen || a < last.lo || a + len > last.hi) {
        std::shared_lock<std::shared_mutex> lk(g_pin_m);
        auto it = std::upper_bound(g_pins.begin(), g_pins.end(), a,
                                   [](uintptr_t v, const pinned_range& r) { return v < r.lo; });
        if (it == g_pins.begin()) return nullptr;
        --it;
        if (a + len > it->hi) return nullptr;
        last = *it;
        last_gen = gen;
    }
    return last.dev + (a - last.lo);
}

// Unmask launch after a scan of the same buffer.
int unmask_impl(hvws_ctx* c, uint8_t* d_rx, uint64_t rx_len) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!c->have_scan) return set_err(HVWS_EINVAL, "hvws_unmask without a preceding hvws_scan");
    if (d_rx != c->rx || rx_len != c->rx_len)
        return set_err(HVWS_EINVAL, "hvws_unmask buffer differs from the scanned one");
    // After a RUN step its descriptors are spent (the repair cleared the
    // failure words): a further unmask of the batch goes through the exact
    // frame table, built now, so every frame is XORed again.
    if (c->run_active && (rc = run_materialize(c)) != HVWS_OK) return rc;
    HIP_OR(issue_unmask(c, d_rx, rx_len), HVWS_EHIP);
    return HVWS_OK;
}

void stall_fn(void* usec) { usleep((useconds_t)(uintptr_t)usec); }


// Every live context (hvws_debug_dump).
std::mutex g_ctx_m;
std::vector<hvws_ctx*> g_ctx_all;

int g_bt_fd = 2;
std::atomic<int> g_bt_done{0};

void bt_handler(int) {
    void* fr[64];
    const int n = backtrace(fr, 64);
    char hdr[64];
    const int l = snprintf(hdr, sizeof(hdr), "--- thread %ld\n", (long)syscall(SYS_gettid));
    if (l > 0) (void)!write(g_bt_fd, hdr, (size_t)l);
    backtrace_symbols_fd(fr, n, g_bt_fd);
    g_bt_done.fetch_add(1, std::memory_order_release);
}

const char* qname(hipError_t q) {
    return q == hipSuccess ? "idle" : q == hipErrorNotReady ? "busy" : hipGetErrorString(q);
}

}  // namespace

// ===================================================================== C ABI
extern "C" {

int hvws_debug_dump(int fd) {
    std::vector<hvws_ctx*> all;
    {
        std::lock_guard<std::mutex> lk(g_ctx_m);
        all = g_ctx_all;
    }
    dprintf(fd, "libhvws: %zu contexts, %d with a worker stream; holding %llu device bytes, %llu pinned bytes\n",
            all.size(), g_door_count.load(), (unsigned long long)g_dev_bytes.load(),
            (unsigned long long)g_pin_bytes.load());
    // memory state first (no HIP call, no lock a stuck caller could hold)
    for (hvws_ctx* c : all) {
        dprintf(fd, "  ctx %p dev %d door_mode %d door_live %d door_seq %llu epoch %llu launches %llu calls %llu",
                (void*)c, c->device, c->door_mode, (int)c->door_live, (unsigned long long)c->door_seq,
                (unsigned long long)c->door_epoch, (unsigned long long)c->door_launches,
                (unsigned long long)c->door_calls);
        if (c->h_door.p) {
            const ddoor* b = c->h_door.as<ddoor>();
            dprintf(fd, " | mailbox%s seq %llu done %llu alive %llu exited %llu served %llu op %u",
                    c->d_door_req ? " (request in device memory)" : "",
                    (unsigned long long)__atomic_load_n(&door_req(c)->seq, __ATOMIC_ACQUIRE),
                    (unsigned long long)__atomic_load_n(&b->done, __ATOMIC_ACQUIRE),
                    (unsigned long long)__atomic_load_n(&b->alive, __ATOMIC_ACQUIRE),
                    (unsigned long long)__atomic_load_n(&b->exited, __ATOMIC_ACQUIRE),
                    (unsigned long long)__atomic_load_n(&b->served, __ATOMIC_ACQUIRE), door_req(c)->op);
        }
        const char* at = c->at.load();
        dprintf(fd, " | wedged %d broken %d | in %s | last scan path %d, have_scan %d\n", (int)c->door_wedged,
                (int)c->door_broken, at ? at : "-", c->scan_path, (int)c->have_scan);
    }
    dprintf(fd, "libhvws: worker launches wedged %llu, requests unanswered %llu (process)\n",
            (unsigned long long)g_door_wedged.load(), (unsigned long long)g_door_failed.load());
    for (hvws_ctx* c : all) {
        if (c->at.load()) {   // its streams may be going away under that call: not queried
            dprintf(fd, "  ctx %p streams: not queried (in %s)\n", (void*)c, c->at.load());
            continue;
        }
        dprintf(fd, "  ctx %p streams:", (void*)c);
        const struct {
            const char* n;
            hipStream_t s;
        } ss[] = {{"stream", c->stream}, {"sstream", c->sstream}, {"copy_in", c->copy_in},
                  {"copy_out", c->copy_out}};
        for (const auto& x : ss)
            if (x.s) dprintf(fd, " %s=%s", x.n, qname(hipStreamQuery(x.s)));
        if (c->door_q)
            dprintf(fd, " worker-queue=%s error=0x%x", door_queue_idle(c->door_q) ? "idle" : "running",
                    door_queue_error(c->door_q));
        dprintf(fd, "\n");
    }
    return (int)all.size();
}

int hvws_debug_backtraces(int fd) {
    struct sigaction sa = {}, old = {};
    sa.sa_handler = bt_handler;
    sigemptyset(&sa.sa_mask);
    sa.sa_flags = SA_RESTART;
    void* warm[4];
    (void)backtrace(warm, 4);   // loads the unwinder outside the handler
    g_bt_fd = fd;
    if (sigaction(SIGUSR2, &sa, &old) != 0) return -1;
    const long self = (long)syscall(SYS_gettid);
    int answered = 0;
    if (DIR* d = opendir("/proc/self/task")) {
        while (dirent* e = readdir(d)) {
            const long tid = atol(e->d_name);
            if (tid <= 0) continue;
            if (tid == self) {
                dprintf(fd, "--- thread %ld (the caller)\n", tid);
                continue;
            }
            const int before = g_bt_done.load(std::memory_order_acquire);
            if (syscall(SYS_tgkill, getpid(), tid, SIGUSR2) != 0) continue;
            for (int i = 0; i < 200 && g_bt_done.load(std::memory_order_acquire) == before; ++i) usleep(1000);
            if (g_bt_done.load(std::memory_order_acquire) != before) ++answered;
            else dprintf(fd, "--- thread %ld: no answer\n", tid);
        }
        closedir(d);
    }
    // A thread that had SIGUSR2 blocked, or sat in a long system call, takes
    // it after this returns: with the default action (terminate) restored,
    // that would kill a healthy process from its own diagnostics (advisor
    // r4).  So the handler stays installed unless the program had one.
    if (old.sa_handler != SIG_DFL || (old.sa_flags & SA_SIGINFO)) sigaction(SIGUSR2, &old, nullptr);
    return answered;
}


const char* hvws_last_error(void) { return g_err; }

int hvws_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int hvws_device_identity(int device, char* bus_id, int len, int* cur) {
    if (!bus_id || len < 13) return set_err(HVWS_EINVAL, "bus id buffer too small");
    HIP_OR(hipSetDevice(device), HVWS_EHIP);
    int d = -1;
    HIP_OR(hipGetDevice(&d), HVWS_EHIP);
    if (cur) *cur = d;
    HIP_OR(hipDeviceGetPCIBusId(bus_id, len, d), HVWS_EHIP);
    return HVWS_OK;
}

hvws_ctx* hvws_ctx_create(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_err(HVWS_ENODEV, "no HIP device available (%s)", e != hipSuccess ? hipGetErrorString(e) : "count 0");
        return nullptr;
    }
    if (device < 0 || device >= n) {
        set_err(HVWS_EINVAL, "device %d out of range (have %d)", device, n);
        return nullptr;
    }
    if ((e = hipSetDevice(device)) != hipSuccess) {
        set_err(HVWS_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
        return nullptr;
    }
    hvws_ctx* c = new hvws_ctx();
    c->device = device;
    {
        std::lock_guard<std::mutex> lk(g_ctx_m);
        g_ctx_all.push_back(c);
    }
    // Tables the device reads (upload slots) or writes (check verdict) in
    // host memory while the host uses them between launches: fine-grained,
    // so no stale copy can sit in a device cache across reuses.
    for (hbuf& b : c->h_up) b.flags = hipHostMallocCoherent;
    c->h_status.flags = hipHostMallocCoherent;
    c->h_small_done.flags = hipHostMallocCoherent;
    if (const char* sp = experiment("small_poll")) c->small_poll = atoi(sp) ? 1 : 0;
    if (const char* zc = experiment("small_zc")) c->small_zc = atoi(zc) ? 1 : 0;
    if (const char* zb = experiment("zc_batch")) c->zc_batch = strtoull(zb, nullptr, 0);
    if (const char* sp = experiment("spec")) c->spec_mode = atoi(sp) == 0 ? 0 : (atoi(sp) == 1 ? 1 : (atoi(sp) == 2 ? 2 : -1));
    if (const char* wv = experiment("walk_verify")) c->verify_mode = atoi(wv) < 0 ? -1 : (atoi(wv) ? 1 : 0);
    // The pipelined scan stream at the highest priority: a scan kernel of
    // ~1000 workgroups queued while an unmask grid is being dispatched waits
    // for that whole grid at normal priority, but is dispatched beside it at
    // high priority (scripts/dispatch_probe.hip).
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    const int scan_prio = prio_greatest;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithPriority(&c->sstream, hipStreamNonBlocking, scan_prio) != hipSuccess) {
        set_err(HVWS_EHIP, "stream creation failed");
        hvws_ctx_destroy(c);
        return nullptr;
    }
    bool ev_ok = true;
    for (auto& ev : c->ev) ev_ok = ev_ok && hipEventCreate(&ev) == hipSuccess;
    for (auto& row : c->tev)
        for (auto& ev : row) ev_ok = ev_ok && hipEventCreate(&ev) == hipSuccess;
    for (auto& ev : c->up_ev) ev_ok = ev_ok && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
    for (tset& t : c->ts) ev_ok = ev_ok && hipEventCreateWithFlags(&t.free_ev, hipEventDisableTiming) == hipSuccess;
    ev_ok = ev_ok && hipEventCreateWithFlags(&c->scan_done, hipEventDisableTiming) == hipSuccess;
    c->cs = c->stream;
    if (!ev_ok) {
        set_err(HVWS_EHIP, "event creation failed");
        hvws_ctx_destroy(c);
        return nullptr;
    }
    return c;
}

void hvws_ctx_destroy(hvws_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    door_release(c);
    // Each runtime call of the teardown is named while it runs (c->at): a
    // teardown that hangs names its call in the wedge report and
    // hvws_debug_dump (round 5: the r4k hang was inside this teardown).
    const auto passes = [c](rel ph) {   // each pass releases what it declares, phase by phase
        c->u8.release(ph);
        c->mg.release(ph);
        c->sd.release(ph);
        c->rp.release(ph);
        c->fan.release(ph);
        c->rt.release(ph);
        c->rn.release(ph);
        c->en.release(ph);
        c->sq.release(ph);
        c->bg.release(ph);
        c->subs.release(ph);
        c->ck.release(ph);
        c->tx.release(ph);
    };
    {
        in_call ic(c, "hipStreamSynchronize(stream)");
        if (c->stream) hipStreamSynchronize(c->stream);
    }
    {
        in_call ic(c, "hipStreamSynchronize(sstream)");
        if (c->sstream) hipStreamSynchronize(c->sstream);
    }
    {
        in_call ic(c, "hipFree (table sets)");
        for (tset& t : c->ts) t.release();
    }
    {
        in_call ic(c, "hipFree (scratch, sieve, pipeline, staging)");
        free_all({&c->sl_hdr, &c->sl_off, &c->sl_len, &c->sl_length, &c->sl_key, &c->sl_keyrot, &c->sl_info, &c->sl_bx});
        free_all({&c->sv_state, &c->sv_tcount, &c->sv_tbase, &c->sv_slot, &c->sv_pool, &c->sv_keep, &c->sv_kbase,
                  &c->sv_Spre, &c->sv_S, &c->sv_J0, &c->sv_J1, &c->sv_mark, &c->sv_hops, &c->sv_rank, &c->sv_cnt,
                  &c->sv_tmp, &c->sv_scr});
        free_all({&c->pipe_slot[0], &c->pipe_slot[1], &c->pipe_slot[2], &c->pipe_segs});
        free_all({&c->segs, &c->carry_in, &c->stage, &c->xor_stage, &c->synth_sizes, &c->synth_tiles, &c->synth_bad,
                  &c->d_small_in, &c->d_small_slots, &c->d_small_ctr});
        passes(REL_DEVICE);
        c->chk.release();
    }
    {
        in_call ic(c, "hipHostFree (pinned buffers)");
        c->h_sv.release();
        c->h_small_in.release();
        c->h_small_done.release();
        c->h_small_out.release();
        c->h_feed.release();
        passes(REL_PINNED);
        c->h_segs.release();
        for (hbuf& b : c->h_up) b.release();
        c->h_total.release();
        c->h_chk.release();
        c->h_readback.release();
        c->h_status.release();
    }
    {
        in_call ic(c, "hipEventDestroy");
        for (tset& t : c->ts)
            if (t.free_ev) hipEventDestroy(t.free_ev);
        if (c->sv_ev) hipEventDestroy(c->sv_ev);
        passes(REL_EVENTS);
        for (hipEvent_t ev : c->pipe_ev)
            if (ev) hipEventDestroy(ev);
        for (auto& ev : c->ev)
            if (ev) hipEventDestroy(ev);
        for (auto& row : c->tev)
            for (auto& ev : row)
                if (ev) hipEventDestroy(ev);
        for (auto& ev : c->up_ev)
            if (ev) hipEventDestroy(ev);
        for (auto& ev : c->span_ev)
            if (ev) hipEventDestroy(ev);
        if (c->scan_done) hipEventDestroy(c->scan_done);
    }
    {
        in_call ic(c, "hipStreamDestroy (context streams)");
        if (c->stream) hipStreamDestroy(c->stream);
        if (c->copy_in) hipStreamDestroy(c->copy_in);
        if (c->copy_out) hipStreamDestroy(c->copy_out);
        if (c->sstream) hipStreamDestroy(c->sstream);
    }
    {
        std::lock_guard<std::mutex> lk(g_ctx_m);
        g_ctx_all.erase(std::remove(g_ctx_all.begin(), g_ctx_all.end(), c), g_ctx_all.end());
    }
    delete c;
}

void* hvws_ctx_stream(hvws_ctx* c) { return c ? (void*)c->stream : nullptr; }
int hvws_ctx_device(hvws_ctx* c) { return c ? c->device : -1; }

void* hvws_dev_alloc(hvws_ctx* c, uint64_t bytes) {
    if (check_ctx(c) != HVWS_OK) return nullptr;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) {
        set_err(HVWS_ENOMEM, "hipMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
        return nullptr;
    }
    return p;
}

void hvws_dev_free(hvws_ctx* c, void* p) {
    if (!c || !p) return;
    hipSetDevice(c->device);
    door_park_device();
    // The runtime holds the buffers of the last kernel dispatched on a stream
    // until the next dispatch there: without an empty launch on each of the
    // context's compute streams, a freed 68.7 GB batch stayed allocated.
    for (hipStream_t s : {c->stream, c->sstream})
        if (s && launch_noop(s) != hipSuccess) (void)hipGetLastError();
    hipStreamSynchronize(c->stream);
    if (c->sstream) hipStreamSynchronize(c->sstream);
    hipFree(p);
}

void* hvws_host_alloc(hvws_ctx* c, uint64_t bytes) {
    if (check_ctx(c) != HVWS_OK) return nullptr;
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault);
    if (e != hipSuccess) {
        set_err(HVWS_ENOMEM, "hipHostMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
        return nullptr;
    }
    if (uint8_t* dev = host_mapped(p)) pin_add(p, bytes ? bytes : 16, dev, false);
    return p;
}

void hvws_host_free(hvws_ctx* c, void* p) {
    if (!c || !p) return;
    hipSetDevice(c->device);
    door_park_device();
    pin_remove(p);
    hipHostFree(p);
}

int hvws_host_register(hvws_ctx* c, void* p, uint64_t bytes) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!p || !bytes) return set_err(HVWS_EINVAL, "empty range");
    HIP_OR(hipHostRegister(p, bytes, hipHostRegisterMapped), HVWS_EHIP);
    uint8_t* dev = host_mapped(p);
    if (!dev) {
        hipHostUnregister(p);
        return set_err(HVWS_EHIP, "registered range not device-mapped");
    }
    pin_add(p, bytes, dev, true);
    return HVWS_OK;
}

int hvws_host_unregister(hvws_ctx* c, void* p) {
    int rc = check_ctx(c);
    if (rc) return rc;
    const pinned_range r = pin_remove(p);
    if (!r.lo || !r.registered) return set_err(HVWS_EINVAL, "not a range from hvws_host_register");
    door_park_device();
    HIP_OR(hipHostUnregister(p), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_rx_reads(hvws_ctx* c, char* const* reads, const uint64_t* lens, websocket_parser* carry, uint32_t n,
                  int unmask) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (n && (!reads || !lens)) return set_err(HVWS_EINVAL, "null read table");
    if (n == 0) return set_err(HVWS_EINVAL, "no reads");
    // In-place reads exist only on the small path: with it switched off
    // (hvws_set_small_batch_limit ~0) callers fall back to the general path.
    if (c->small_limit == ~0ull) return set_err(HVWS_EINVAL, "small-batch path disabled on this context");
    // device address of every read; the batch goes to k_small in address order
    std::vector<uint8_t*> dev(n);
    bool sorted = true;
    for (uint32_t i = 0; i < n; ++i) {
        if (lens[i] > kStageSegment)
            return set_err(HVWS_EINVAL, "read %u: %llu bytes (at most %llu)", i, (unsigned long long)lens[i],
                           (unsigned long long)kStageSegment);
        if (!(dev[i] = pinned_dev(reads[i], lens[i])))
            return set_err(HVWS_EINVAL, "read %u is not in registered pinned memory", i);
        if (i && dev[i] < dev[i - 1]) sorted = false;
    }
    std::vector<uint32_t> ord(n);
    for (uint32_t i = 0; i < n; ++i) ord[i] = i;
    if (!sorted) std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return dev[a] < dev[b]; });
    uint8_t* base = n ? (uint8_t*)((uintptr_t)dev[ord[0]] & ~(uintptr_t)15) : nullptr;
    std::vector<hvws_segment> segs(n);
    std::vector<websocket_parser> cin(carry ? n : 0);
    uint64_t span = 0, total = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = ord[k];
        segs[k].off = (uint64_t)(dev[i] - base);
        segs[k].len = lens[i];
        if (k && segs[k].off < segs[k - 1].off + segs[k - 1].len)
            return set_err(HVWS_EINVAL, "reads %u and %u overlap", ord[k - 1], i);
        span = segs[k].off + lens[i];
        total += lens[i];
        if (carry) copy_parser(cin[k], carry[i]);
    }
    const uint64_t limit = c->small_limit ? c->small_limit : kSmallBatch;
    if (total > limit) return set_err(HVWS_EINVAL, "%llu bytes of reads (at most %llu per call)",
                                      (unsigned long long)total, (unsigned long long)limit);
    if ((rc = rx_batch_small(c, nullptr, span, segs.data(), carry ? cin.data() : nullptr, n, unmask, base)) != HVWS_OK)
        return rc;
    // results back in caller order, offsets relative to each read; reads
    // already in address order (one arena filled in order) rebase in place
    if (sorted) {
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t rb = segs[i].off;
            hvws_frame* r = c->hcache.data() + c->hfirst[i];
            for (uint64_t j = 0; j < c->hcount[i]; ++j) {
                if (r[j].hdr_off >= 0) r[j].hdr_off -= (int64_t)rb;
                r[j].pay_off -= rb;
            }
            if (carry) {
                void* keep = carry[i].data;
                copy_parser(carry[i], cin[i]);
                carry[i].data = keep;
            }
        }
        return HVWS_OK;
    }
    std::vector<hvws_frame> recs(c->hcache.size());
    std::vector<uint64_t> first(n), count(n);
    std::vector<dcarry> hc(n);
    uint64_t at = 0;
    std::vector<uint32_t> pos(n);   // caller index -> address-order position
    for (uint32_t k = 0; k < n; ++k) pos[ord[k]] = k;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = pos[i];
        const uint64_t cnt = c->hcount[k], rb = segs[k].off;
        first[i] = at;
        count[i] = cnt;
        hc[i] = c->hcarry[k];
        for (uint64_t j = 0; j < cnt; ++j) {
            hvws_frame r = c->hcache[c->hfirst[k] + j];
            if (r.hdr_off >= 0) r.hdr_off -= (int64_t)rb;
            r.pay_off -= rb;
            recs[at + j] = r;
        }
        at += cnt;
        if (carry) {
            void* keep = carry[i].data;
            copy_parser(carry[i], cin[k]);
            carry[i].data = keep;
        }
    }
    c->hcache.swap(recs);
    c->hfirst.swap(first);
    c->hcount.swap(count);
    c->hcarry.swap(hc);
    return HVWS_OK;
}

int hvws_h2d(hvws_ctx* c, void* dst, const void* src, uint64_t n) {
    int rc = check_ctx(c);
    if (rc) return rc;
    HIP_OR(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_d2h(hvws_ctx* c, void* dst, const void* src, uint64_t n) {
    int rc = check_ctx(c);
    if (rc) return rc;
    HIP_OR(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->stream), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_memset(hvws_ctx* c, void* dst, int v, uint64_t n) {
    int rc = check_ctx(c);
    if (rc) return rc;
    HIP_OR(hipMemsetAsync(dst, v, n, c->stream), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_d2d(hvws_ctx* c, void* dst, const void* src, uint64_t n) {
    int rc = check_ctx(c);
    if (rc) return rc;
    HIP_OR(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, c->stream), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_sync(hvws_ctx* c) {
    int rc = check_ctx(c);
    if (rc) return rc;
    HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(c->sstream), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_debug_stall(hvws_ctx* c, uint32_t usec) {
    int rc = check_ctx(c);
    if (rc) return rc;
    HIP_OR(hipLaunchHostFunc(c->stream, stall_fn, (void*)(uintptr_t)usec), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_scan(hvws_ctx* c, const uint8_t* d_rx, uint64_t rx_len, const hvws_segment* segs,
              const websocket_parser* carry_in, uint32_t nseg) {
    int rc = check_batch_args(c, d_rx, segs, nseg);
    if (rc) return rc;
    if ((rc = upload_segments(c, segs, carry_in, nseg, rx_len)) != HVWS_OK) return rc;
    return scan_device_carry(c, d_rx, rx_len, nseg);
}

int hvws_unmask(hvws_ctx* c, uint8_t* d_rx, uint64_t rx_len) { return unmask_impl(c, d_rx, rx_len); }

// UTF-8 validation over the last scan's frame table (hvws_utf8.hip): tile
// index at U8_TILE, words, fold -- all on the context stream, behind the scan
// (and the unmask of a step), reading rx and the current table set only.
int hvws_utf8(hvws_ctx* c, const uint8_t* d_rx, uint64_t rx_len, int masked, const uint32_t* state_in) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if ((rc = behind_scan(c, "hvws_utf8", d_rx, rx_len)) != HVWS_OK) return rc;
    // a RUN step left no frame table: build it now (as hvws_unmask does)
    if (c->run_active && (rc = run_materialize(c)) != HVWS_OK) return rc;
    const uint32_t nseg = c->nseg;
    const uint64_t cap = record_bound(c);
    const uint64_t ntiles = (rx_len + U8_TILE - 1) / U8_TILE;
    HIP_OR(c->u8.words.ensure(cap * 4 + 16), HVWS_ENOMEM);
    HIP_OR(c->u8.flags.ensure_zeroed(cap * 4 + 16, c->stream), HVWS_ENOMEM);
    HIP_OR(c->u8.tiles.ensure((ntiles + 8) * 4), HVWS_ENOMEM);
    HIP_OR(c->u8.meta.ensure(64), HVWS_ENOMEM);
    HIP_OR(c->u8.in.ensure((uint64_t)nseg * 4 + 16), HVWS_ENOMEM);
    HIP_OR(c->u8.out.ensure((uint64_t)nseg * 4 + 16), HVWS_ENOMEM);
    HIP_OR(c->u8.bad.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    if ((rc = c->u8.up.send(c->u8.in.p, c->stream, state_in, (uint64_t)nseg * 4)) != HVWS_OK) return rc;
    HIP_OR(timed_begin(c), HVWS_EHIP);
    if (ntiles)
        HIP_OR(launch_tile_index(c->T().f_off.as<uint64_t>(), c->T().f_len.as<uint64_t>(), 0, c->T().total.as<uint64_t>(),
                                 c->u8.tiles.as<uint32_t>(), ntiles, U8_TILE, c->stream),
               HVWS_EHIP);
    HIP_OR(launch_utf8(d_rx, rx_len, c->T().f_off.as<uint64_t>(), c->T().f_len.as<uint64_t>(),
                       c->T().f_keyrot.as<uint32_t>(), c->T().f_info.as<uint32_t>(), c->T().total.as<uint64_t>(), cap,
                       c->u8.tiles.as<uint32_t>(), ntiles, masked, c->u8.flags.as<uint32_t>(),
                       c->u8.words.as<uint32_t>(), c->u8.meta.as<uint64_t>(), c->T().counts.as<uint64_t>(),
                       c->T().bases.as<uint64_t>(), nseg, state_in ? c->u8.in.as<uint32_t>() : nullptr,
                       c->u8.out.as<uint32_t>(), c->u8.bad.as<uint64_t>(), c->stream),
           HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    HIP_OR(hold_tables(c), HVWS_EHIP);
    c->u8.have = true;
    c->u8.nseg = nseg;
    c->u8.gen = c->scan_gen;
    return HVWS_OK;
}

int64_t hvws_utf8_count(hvws_ctx* c) {
    if (!c || !c->u8.have || check_ctx(c) != HVWS_OK) return -1;
    return read_count(c, c->u8.meta.as<uint64_t>(), "hvws_utf8_count");
}

int hvws_get_utf8_words(hvws_ctx* c, uint32_t* out, uint64_t first, uint64_t n) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->u8.have) return set_err(HVWS_EINVAL, "no hvws_utf8 call yet");
    const int64_t have = hvws_utf8_count(c);
    if (have < 0) return HVWS_EHIP;
    const uint64_t nrec = (uint64_t)have;
    if (first > nrec || n > nrec - first) return set_err(HVWS_EINVAL, "word range out of bounds");
    if (n == 0) return HVWS_OK;
    if (!out) return set_err(HVWS_EINVAL, "null output");
    return read_rows(c, {{out, c->u8.words.as<uint32_t>() + first, n * 4}});
}

int hvws_get_utf8(hvws_ctx* c, uint32_t* state_out, uint64_t* bad) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->u8.have) return set_err(HVWS_EINVAL, "no hvws_utf8 call yet");
    const uint64_t nseg = c->u8.nseg;
    return read_rows(c, {{state_out, c->u8.out.p, nseg * 4}, {bad, c->u8.bad.p, nseg * 8}});
}

uint64_t hvws_utf8_tile(void) { return U8_TILE; }

static_assert(sizeof(dmsg) == sizeof(hvws_msg) && sizeof(dmsg) == 40, "dmsg mirrors hvws_msg");
static_assert(sizeof(dmsg_state) == sizeof(hvws_msg_state) && sizeof(dmsg_state) == 16,
              "dmsg_state mirrors hvws_msg_state");
static_assert(M_END == HVWS_M_END && M_CONT == HVWS_M_CONT && M_CTL == HVWS_M_CTL, "piece bits");
static_assert(sizeof(drfc_state) == sizeof(hvws_rfc_state) && sizeof(drfc_state) == 48,
              "drfc_state mirrors hvws_rfc_state");

// Message reassembly over the last scan's frame table (hvws_msg.hip): the
// table pass, the tile index over the output, the gather -- all on the context
// stream, behind the scan (and the unmask of a step), reading rx and the
// current table set only.  prev != nullptr: the joined form
// (hvws_messages_joined), whose tables are over rows -- per segment its carried
// span in prev->d, then its records -- and which may run with up to nseg pieces
// more than records.  rfc: the RFC form (hvws_messages_rfc), the joined form
// over two virtual connections per connection -- vn states and offsets, 2s the
// data class's and 2s + 1 the control class's.
namespace {
struct msg_prev {
    const uint8_t* d;
    uint64_t len;
    const uint64_t* off;   // host, nseg words
};

int messages_pass(hvws_ctx* c, const uint8_t* d_rx, uint64_t rx_len, int masked, uint8_t* d_out, uint64_t out_cap,
                  const hvws_msg_state* state_in, const msg_prev* prev, bool rfc = false) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if ((rc = behind_scan(c, "hvws_messages", d_rx, rx_len)) != HVWS_OK) return rc;
    if (!d_out || ((uintptr_t)d_out & 15u) != 0)
        return set_err(HVWS_EINVAL, "hvws_messages: d_out must be 16-byte aligned");
    {
        const uintptr_t o = (uintptr_t)d_out, r = (uintptr_t)d_rx;
        if (o < r + rx_len && r < o + out_cap) return set_err(HVWS_EINVAL, "hvws_messages: d_out overlaps the batch");
    }
    const uint32_t nseg = c->nseg;
    const uint64_t vn = rfc ? 2ull * nseg : nseg;   // states: one per (virtual) connection
    if (state_in)
        for (uint64_t s = 0; s < vn; ++s)
            if ((state_in[s].open == 0 && state_in[s].pending != 0) || state_in[s].opcode > 15)
                return set_err(HVWS_EINVAL, "hvws_messages: state_in is no state hvws_get_msg_state returns");
    // The joined form: every carried range inside prev, the output clear of it;
    // carried = the sum of the pending bytes, saturating.
    uint64_t carried = 0;
    if (prev) {
        if (((uintptr_t)prev->d & 15u) != 0)
            return set_err(HVWS_EINVAL, "hvws_messages_joined: d_prev must be 16-byte aligned");
        if (state_in)
            for (uint64_t s = 0; s < vn; ++s) {
                const uint64_t P = state_in[s].pending;
                if (P == 0) continue;
                if (!prev->d || !prev->off)
                    return set_err(HVWS_EINVAL, "hvws_messages_joined: pending bytes without d_prev / prev_off");
                if (prev->off[s] > prev->len || P > prev->len - prev->off[s])
                    return set_err(HVWS_EINVAL, "hvws_messages_joined: a carried range leaves d_prev");
                carried = P > UINT64_MAX - carried ? UINT64_MAX : carried + P;
            }
        const uintptr_t o = (uintptr_t)d_out, p = (uintptr_t)prev->d;
        if (prev->d && o < p + prev->len && p < o + out_cap)
            return set_err(HVWS_EINVAL, "hvws_messages_joined: d_out overlaps d_prev");
    }
    const bool rows = prev && nseg;   // without segments there is no carried row: the plain tables
    // a RUN step left no frame table: build it now (as hvws_unmask does)
    if (c->run_active && (rc = run_materialize(c)) != HVWS_OK) return rc;
    const uint64_t cap = record_bound(c);
    const uint64_t ncap = rows ? cap + vn : cap;   // rows, and the bound of the pieces
    // the output cannot exceed the batch and what is carried
    const uint64_t need = carried > UINT64_MAX - rx_len ? UINT64_MAX : rx_len + carried;
    const uint64_t bound = std::min(need, out_cap);
    const int geom = msg_variant(need, cap);
    const uint64_t tile = msg_gather_tile(geom);
    uint64_t ntiles = (bound + tile - 1) / tile;
    HIP_OR(c->mg.scan.ensure(msg_scratch_bytes(ncap)), HVWS_ENOMEM);
    HIP_OR(c->mg.off.ensure(ncap * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->mg.tiles.ensure((ntiles + 8) * 4), HVWS_ENOMEM);
    HIP_OR(c->mg.msgs.ensure((ncap + 1) * sizeof(dmsg)), HVWS_ENOMEM);
    HIP_OR(c->mg.first.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->mg.count.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    // state_in, then (joined) prev_off
    HIP_OR(c->mg.in.ensure(vn * (sizeof(dmsg_state) + 8) + 16), HVWS_ENOMEM);
    HIP_OR(c->mg.out.ensure((uint64_t)nseg * (rfc ? sizeof(drfc_state) : sizeof(dmsg_state)) + 16), HVWS_ENOMEM);
    HIP_OR(c->mg.meta.ensure(64), HVWS_ENOMEM);
    if (rows) {
        HIP_OR(c->mg.row_len.ensure(ncap * 8 + 16), HVWS_ENOMEM);
        HIP_OR(c->mg.row_src.ensure(ncap * 8 + 16), HVWS_ENOMEM);
        HIP_OR(c->mg.row_key.ensure(ncap * 4 + 16), HVWS_ENOMEM);
        HIP_OR(c->mg.row_info.ensure(ncap * 4 + 16), HVWS_ENOMEM);
        HIP_OR(c->mg.prow.ensure((ncap + 1) * 8), HVWS_ENOMEM);
        HIP_OR(c->mg.carry.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    }
    if (rows && rfc) {
        HIP_OR(c->mg.cls.ensure(msg_cls_bytes(cap)), HVWS_ENOMEM);
        HIP_OR(c->mg.rec.ensure(ncap * 8 + 16), HVWS_ENOMEM);
        HIP_OR(c->mg.vbase.ensure(vn * 8 + 16), HVWS_ENOMEM);
        HIP_OR(c->mg.vcnt.ensure(vn * 8 + 16), HVWS_ENOMEM);
    }
    c->mg.have = false;   // the tables are being rewritten
    c->mg.joined = false;
    c->mg.rfc = false;
    c->rp.have = false;   // ... which a reply table indexes
    const bool with_off = rows && carried;   // prev_off rides behind the states in the same slot
    if ((rc = c->mg.up.send(c->mg.in.p, c->stream, state_in, vn * sizeof(dmsg_state), with_off ? prev->off : nullptr,
                            with_off ? vn * 8 : 0)) != HVWS_OK)
        return rc;
    const msg_rows mr{c->mg.row_len.as<uint64_t>(), c->mg.row_src.as<uint64_t>(), c->mg.row_key.as<uint32_t>(),
                      c->mg.row_info.as<uint32_t>(), c->mg.prow.as<uint64_t>()};
    HIP_OR(timed_begin(c), HVWS_EHIP);
    if (rows) {
        const dframes fr{nullptr, c->T().f_off.as<uint64_t>(), c->T().f_len.as<uint64_t>(), nullptr, nullptr,
                         c->T().f_keyrot.as<uint32_t>(), c->T().f_info.as<uint32_t>(), cap};
        const uint64_t* d_prev_off =
            with_off ? reinterpret_cast<const uint64_t*>((uint8_t*)c->mg.in.p + vn * sizeof(dmsg_state)) : nullptr;
        if (rfc) {
            const rfc_rows rr{c->mg.rec.as<uint64_t>(), c->mg.vbase.as<uint64_t>(), c->mg.vcnt.as<uint64_t>()};
            HIP_OR(launch_msg_table_rfc(fr, masked, c->T().total.as<uint64_t>(), cap, c->T().bases.as<uint64_t>(), nseg,
                                        state_in ? c->mg.in.as<dmsg_state>() : nullptr, d_prev_off, c->mg.scan.p,
                                        c->mg.cls.p, mr, rr, c->mg.off.as<uint64_t>(), c->mg.msgs.as<dmsg>(),
                                        c->mg.first.as<uint64_t>(), c->mg.count.as<uint64_t>(),
                                        c->mg.out.as<drfc_state>(), c->mg.meta.as<uint64_t>(), c->stream),
                   HVWS_EHIP);
        } else {
            HIP_OR(launch_msg_table_joined(fr, masked, c->T().total.as<uint64_t>(), cap, c->T().counts.as<uint64_t>(),
                                           c->T().bases.as<uint64_t>(), nseg,
                                           state_in ? c->mg.in.as<dmsg_state>() : nullptr, d_prev_off, c->mg.scan.p,
                                           mr, c->mg.off.as<uint64_t>(), c->mg.msgs.as<dmsg>(),
                                           c->mg.first.as<uint64_t>(), c->mg.count.as<uint64_t>(),
                                           c->mg.out.as<dmsg_state>(), c->mg.carry.as<uint64_t>(),
                                           c->mg.meta.as<uint64_t>(), c->stream),
                   HVWS_EHIP);
        }
    } else {
        HIP_OR(launch_msg_table(c->T().f_len.as<uint64_t>(), c->T().f_info.as<uint32_t>(), c->T().total.as<uint64_t>(),
                                cap, c->T().counts.as<uint64_t>(), c->T().bases.as<uint64_t>(), nseg,
                                state_in ? c->mg.in.as<dmsg_state>() : nullptr, c->mg.scan.p, c->mg.off.as<uint64_t>(),
                                c->mg.msgs.as<dmsg>(), c->mg.first.as<uint64_t>(), c->mg.count.as<uint64_t>(),
                                c->mg.out.as<dmsg_state>(), c->mg.meta.as<uint64_t>(), c->stream),
               HVWS_EHIP);
    }
    bool fits = true;
    if (out_cap < need) {   // the one wait: does the payload fit?
        uint64_t total = 0;
        HIP_OR(read_word(c, c->mg.meta.as<uint64_t>() + 1, &total), HVWS_EHIP);
        fits = total <= out_cap;
        ntiles = (std::min(total, out_cap) + tile - 1) / tile;
    }
    if (fits) {
        // the tile index over the output: by records, or by rows (meta[0] counts either)
        if (ntiles)
            HIP_OR(launch_tile_index(c->mg.off.as<uint64_t>(), rows ? mr.len : c->T().f_len.as<uint64_t>(), 0,
                                     c->mg.meta.as<uint64_t>(), c->mg.tiles.as<uint32_t>(), ntiles, tile, c->stream),
                   HVWS_EHIP);
        if (rows)
            HIP_OR(launch_msg_gather_joined(geom, d_rx, rx_len, prev->d, prev->d ? prev->len : 0, mr,
                                            c->mg.off.as<uint64_t>(), c->mg.tiles.as<uint32_t>(), ntiles,
                                            c->mg.meta.as<uint64_t>(), masked, d_out, out_cap, c->stream),
                   HVWS_EHIP);
        else
            HIP_OR(launch_msg_gather(geom, d_rx, rx_len, c->T().f_off.as<uint64_t>(), c->T().f_len.as<uint64_t>(),
                                     c->T().f_keyrot.as<uint32_t>(), c->mg.off.as<uint64_t>(),
                                     c->mg.tiles.as<uint32_t>(), ntiles, c->mg.meta.as<uint64_t>(), masked, d_out,
                                     out_cap, c->stream),
                   HVWS_EHIP);
    }
    HIP_OR(timed_end(c), HVWS_EHIP);
    HIP_OR(hold_tables(c), HVWS_EHIP);   // even when the payload does not fit: the table pass ran
    if (!fits) return set_err(HVWS_EINVAL, "hvws_messages: the payload does not fit out_cap");
    c->mg.have = true;
    c->mg.joined = prev != nullptr && !rfc;
    c->mg.rfc = rfc;
    c->mg.nseg = nseg;
    c->mg.cap = ncap;
    c->mg.gen = c->scan_gen;
    ++c->mg.seq;
    c->mg.dout = d_out;
    c->mg.out_cap = out_cap;
    return HVWS_OK;
}
}  // namespace

int hvws_messages(hvws_ctx* c, const uint8_t* d_rx, uint64_t rx_len, int masked, uint8_t* d_out, uint64_t out_cap,
                  const hvws_msg_state* state_in) {
    return messages_pass(c, d_rx, rx_len, masked, d_out, out_cap, state_in, nullptr);
}

int hvws_messages_joined(hvws_ctx* c, const uint8_t* d_rx, uint64_t rx_len, int masked, uint8_t* d_out,
                         uint64_t out_cap, const hvws_msg_state* state_in, const uint8_t* d_prev, uint64_t prev_len,
                         const uint64_t* prev_off) {
    const msg_prev prev{d_prev, d_prev ? prev_len : 0, prev_off};
    return messages_pass(c, d_rx, rx_len, masked, d_out, out_cap, state_in, &prev);
}

// The RFC form: the states repacked per virtual connection (2s data, 2s + 1
// control), their offsets into d_prev behind them, then the joined pass.
int hvws_messages_rfc(hvws_ctx* c, const uint8_t* d_rx, uint64_t rx_len, int masked, uint8_t* d_out, uint64_t out_cap,
                      const hvws_rfc_state* state_in, const uint8_t* d_prev, uint64_t prev_len) {
    int rc = check_ctx(c);
    if (rc) return rc;
    const uint32_t nseg = c->nseg;
    if (state_in) {
        c->mg.rf_st.resize(2ull * nseg);
        c->mg.rf_off.resize(2ull * nseg);
        for (uint32_t s = 0; s < nseg; ++s) {
            c->mg.rf_st[2ull * s] = state_in[s].data;
            c->mg.rf_st[2ull * s + 1] = state_in[s].ctl;
            c->mg.rf_off[2ull * s] = state_in[s].data_off;
            c->mg.rf_off[2ull * s + 1] = state_in[s].ctl_off;
        }
    }
    const msg_prev prev{d_prev, d_prev ? prev_len : 0, state_in ? c->mg.rf_off.data() : nullptr};
    return messages_pass(c, d_rx, rx_len, masked, d_out, out_cap, state_in ? c->mg.rf_st.data() : nullptr, &prev, true);
}

int hvws_get_rfc_state(hvws_ctx* c, hvws_rfc_state* out) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.have || !c->mg.rfc) return set_err(HVWS_EINVAL, "no hvws_messages_rfc call yet");
    return read_rows(c, {{out, c->mg.out.p, c->mg.nseg * sizeof(drfc_state)}});
}

int hvws_get_msg_carry(hvws_ctx* c, uint64_t* off) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.have || !c->mg.joined) return set_err(HVWS_EINVAL, "no hvws_messages_joined call yet");
    return read_rows(c, {{off, c->mg.carry.p, (uint64_t)c->mg.nseg * 8}});
}

namespace {
// meta word i of the last hvws_messages (1: payload bytes, 2: pieces); waits
int msg_meta(hvws_ctx* c, int i, uint64_t* v) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.have) return set_err(HVWS_EINVAL, "no hvws_messages call yet");
    HIP_OR(read_word(c, c->mg.meta.as<uint64_t>() + i, v), HVWS_EHIP);
    return HVWS_OK;
}
}  // namespace

int64_t hvws_msg_count(hvws_ctx* c) {
    uint64_t n = 0;
    if (!c || msg_meta(c, 2, &n) != HVWS_OK) return -1;
    return (int64_t)n;
}

int hvws_msg_bytes(hvws_ctx* c, uint64_t* total) {
    if (!total) return set_err(HVWS_EINVAL, "null output");
    return msg_meta(c, 1, total);
}

int hvws_get_messages(hvws_ctx* c, hvws_msg* out, uint64_t first, uint64_t n) {
    uint64_t have = 0;
    int rc = msg_meta(c, 2, &have);
    if (rc) return rc;
    if (first > have || n > have - first) return set_err(HVWS_EINVAL, "piece range out of bounds");
    if (n == 0) return HVWS_OK;
    if (!out) return set_err(HVWS_EINVAL, "null output");
    return read_rows(c, {{out, c->mg.msgs.as<dmsg>() + first, n * sizeof(dmsg)}});
}

int hvws_get_segment_messages(hvws_ctx* c, uint64_t* first, uint64_t* count) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.have) return set_err(HVWS_EINVAL, "no hvws_messages call yet");
    const uint64_t nseg = c->mg.nseg;
    return read_rows(c, {{first, c->mg.first.p, nseg * 8}, {count, c->mg.count.p, nseg * 8}});
}

int hvws_get_msg_state(hvws_ctx* c, hvws_msg_state* out) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->mg.have) return set_err(HVWS_EINVAL, "no hvws_messages call yet");
    if (c->mg.rfc) return set_err(HVWS_EINVAL, "hvws_get_msg_state after hvws_messages_rfc: hvws_get_rfc_state");
    return read_rows(c, {{out, c->mg.out.p, c->mg.nseg * sizeof(dmsg_state)}});
}

const hvws_msg* hvws_messages_device(hvws_ctx* c) {
    if (!c || !c->mg.have) return nullptr;
    return c->mg.msgs.as<hvws_msg>();
}

uint64_t hvws_msg_tile(void) { return MSG_TILE; }

int hvws_step_resident(hvws_ctx* c, uint8_t* d_rx, uint64_t rx_len, const hvws_segment* segs,
                       const websocket_parser* carry_in, uint32_t nseg) {
    int rc = check_batch_args(c, d_rx, segs, nseg);
    if (rc) return rc;
    if (!c->piped) {
        // Entering pipelined mode: both table sets may still be read by work
        // queued on the context stream.
        for (tset& t : c->ts) {
            HIP_OR(hipEventRecord(t.free_ev, c->stream), HVWS_EHIP);
            t.free_wait = t.free_ev;
            t.free_pending = true;
        }
        c->piped = true;
    }
    if ((rc = upload_segments(c, segs, carry_in, nseg, rx_len)) != HVWS_OK) return rc;
    c->cs = c->sstream;
    bool unmasked = false;
    c->run_call = true;
    rc = scan_device_carry(c, d_rx, rx_len, nseg, d_rx, &unmasked);
    c->run_call = false;
    if (rc == HVWS_OK && !unmasked) rc = unmask_impl(c, d_rx, rx_len);
    c->cs = c->stream;
    return rc;
}

int hvws_step(hvws_ctx* c, uint8_t* d_rx, uint64_t rx_len, const hvws_segment* segs,
              const websocket_parser* carry_in, uint32_t nseg) {
    int rc = check_batch_args(c, d_rx, segs, nseg);
    if (rc) return rc;
    if ((rc = upload_segments(c, segs, carry_in, nseg, rx_len)) != HVWS_OK) return rc;
    bool unmasked = false;
    c->run_call = true;
    rc = scan_device_carry(c, d_rx, rx_len, nseg, d_rx, &unmasked);
    c->run_call = false;
    if (rc != HVWS_OK) return rc;
    return unmasked ? HVWS_OK : unmask_impl(c, d_rx, rx_len);
}

int64_t hvws_frame_count(hvws_ctx* c) {
    if (!c || !c->have_scan) return -1;
    if (check_ctx(c) != HVWS_OK || ensure_count(c) != HVWS_OK) return -1;
    return (int64_t)c->nfr;
}

int hvws_get_frames(hvws_ctx* c, hvws_frame* out, uint64_t first, uint64_t n) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!c->have_scan) return set_err(HVWS_EINVAL, "no scan");
    if ((rc = ensure_count(c)) != HVWS_OK) return rc;
    if (first > c->nfr || n > c->nfr - first) return set_err(HVWS_EINVAL, "frame range out of bounds");
    if (n == 0) return HVWS_OK;
    if (c->hcache_valid) {
        memcpy(out, c->hcache.data() + first, n * sizeof(hvws_frame));
        return HVWS_OK;
    }
    std::vector<int64_t> hdr(n);
    std::vector<uint64_t> off(n), len(n), length(n);
    std::vector<uint32_t> key(n), info(n);
    const tset& t = c->T();
    if ((rc = read_rows(c, {{hdr.data(), t.f_hdr.as<int64_t>() + first, n * 8},
                            {off.data(), t.f_off.as<uint64_t>() + first, n * 8},
                            {len.data(), t.f_len.as<uint64_t>() + first, n * 8},
                            {length.data(), t.f_length.as<uint64_t>() + first, n * 8},
                            {key.data(), t.f_key.as<uint32_t>() + first, n * 4},
                            {info.data(), t.f_info.as<uint32_t>() + first, n * 4}})) != HVWS_OK)
        return rc;
    for (uint64_t i = 0; i < n; ++i) {
        out[i].hdr_off = hdr[i];
        out[i].pay_off = off[i];
        out[i].pay_len = len[i];
        out[i].length = length[i];
        out[i].key = key[i];
        out[i].info = info[i];
    }
    return HVWS_OK;
}

int hvws_get_segment_frames(hvws_ctx* c, uint64_t* first, uint64_t* count) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!c->have_scan) return set_err(HVWS_EINVAL, "no scan");
    if ((rc = run_materialize(c)) != HVWS_OK) return rc;
    if (c->hcache_valid) {
        if (first) memcpy(first, c->hfirst.data(), (uint64_t)c->nseg * 8);
        if (count) memcpy(count, c->hcount.data(), (uint64_t)c->nseg * 8);
        return HVWS_OK;
    }
    if (first)
        HIP_OR(hipMemcpyAsync(first, c->T().bases.p, (uint64_t)c->nseg * 8, hipMemcpyDeviceToHost, c->stream),
               HVWS_EHIP);
    if (count)
        HIP_OR(hipMemcpyAsync(count, c->T().counts.p, (uint64_t)c->nseg * 8, hipMemcpyDeviceToHost, c->stream),
               HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_get_carry(hvws_ctx* c, websocket_parser* out, int* started) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!c->have_scan) return set_err(HVWS_EINVAL, "no scan");
    if ((rc = run_materialize(c)) != HVWS_OK) return rc;
    std::vector<dcarry> h;
    const dcarry* src;
    if (c->hcache_valid) {
        src = c->hcarry.data();
    } else {
        h.resize(c->nseg);
        if (c->nseg)
            HIP_OR(hipMemcpyAsync(h.data(), c->T().carry_out.p, (uint64_t)c->nseg * sizeof(dcarry),
                                  hipMemcpyDeviceToHost, c->stream),
                   HVWS_EHIP);
        HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
        src = h.data();
    }
    for (uint32_t s = 0; s < c->nseg; ++s) {
        if (out) from_dcarry(src[s], out[s]);
        if (started) started[s] = (int)src[s].started;
    }
    return HVWS_OK;
}

int hvws_last_times(hvws_ctx* c, float out[2]) {
    int rc = check_ctx(c);
    if (rc) return rc;
    out[0] = out[1] = -1.0f;
    if (!c->have_scan || c->t_seq == 0) return set_err(HVWS_EINVAL, "no scan");
    return step_times_at(c, c->t_cur, out);
}

// Timed region on the device: markers on both compute streams (the scan
// stream and the unmask stream of pipelined steps), so the span runs from
// whichever stream starts first to whichever ends last.
int hvws_span_begin(hvws_ctx* c) {
    int rc = check_ctx(c);
    if (rc) return rc;
    for (auto& ev : c->span_ev)
        if (!ev) HIP_OR(hipEventCreate(&ev), HVWS_EHIP);
    HIP_OR(hipEventRecord(c->span_ev[0], c->stream), HVWS_EHIP);
    HIP_OR(hipEventRecord(c->span_ev[1], c->sstream ? c->sstream : c->stream), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_span_end(hvws_ctx* c, float* ms) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!ms || !c->span_ev[0]) return set_err(HVWS_EINVAL, "no hvws_span_begin");
    HIP_OR(hipEventRecord(c->span_ev[2], c->stream), HVWS_EHIP);
    HIP_OR(hipEventRecord(c->span_ev[3], c->sstream ? c->sstream : c->stream), HVWS_EHIP);
    HIP_OR(hipEventSynchronize(c->span_ev[2]), HVWS_EHIP);
    HIP_OR(hipEventSynchronize(c->span_ev[3]), HVWS_EHIP);
    // max over (begin, end) pairs = latest end - earliest begin
    float best = 0.0f;
    for (int b = 0; b < 2; ++b)
        for (int e = 2; e < 4; ++e) {
            float t = 0.0f;
            HIP_OR(hipEventElapsedTime(&t, c->span_ev[b], c->span_ev[e]), HVWS_EHIP);
            best = std::max(best, t);
        }
    *ms = best;
    return HVWS_OK;
}

int hvws_set_step_event_interval(hvws_ctx* c, uint32_t every) {
    int rc = check_ctx(c);
    if (rc) return rc;
    const int old = (int)c->t_every;
    c->t_every = every;
    return old;
}

int hvws_step_times(hvws_ctx* c, float* out, int max_steps) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!out || max_steps < 0) return set_err(HVWS_EINVAL, "bad output");
    uint64_t n = std::min<uint64_t>(c->t_seq, hvws_ctx::kTimeRing);
    n = std::min<uint64_t>(n, (uint64_t)max_steps);
    for (uint64_t i = 0; i < n; ++i) {
        const int slot = (int)((c->t_seq - n + i) % hvws_ctx::kTimeRing);
        if ((rc = step_times_at(c, slot, out + 2 * i)) != HVWS_OK) return rc;
    }
    return (int)n;
}

int hvws_stream_xor(hvws_ctx* c, uint8_t* d, uint64_t n, uint32_t pattern) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (((uintptr_t)d & 15u) != 0) return set_err(HVWS_EINVAL, "buffer must be 16-byte aligned");
    HIP_OR(launch_stream_xor(unmask_variant_for(n), d, n, pattern, c->stream), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_rx_batch(hvws_ctx* c, uint8_t* h_rx, uint64_t len, const hvws_segment* segs, websocket_parser* carry,
                  uint32_t nseg, int unmask) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!segs && nseg) return set_err(HVWS_EINVAL, "null segment table");
    if (small_eligible(c, len, segs, nseg)) return rx_batch_small(c, h_rx, len, segs, carry, nseg, unmask);
    HIP_OR(c->stage.ensure(len + 64), HVWS_ENOMEM);
    uint8_t* d = c->stage.as<uint8_t>();
    if ((rc = upload_segments(c, segs, carry, nseg, len)) != HVWS_OK) return rc;
    if (len) HIP_OR(hipMemcpyAsync(d, h_rx, len, hipMemcpyHostToDevice, c->stream), HVWS_EHIP);
    bool unmasked = false;
    if ((rc = scan_device_carry(c, d, len, nseg, unmask ? d : nullptr, &unmasked)) != HVWS_OK) return rc;
    if (unmask) {
        if (!unmasked && (rc = unmask_impl(c, d, len)) != HVWS_OK) return rc;
        if (len) HIP_OR(hipMemcpyAsync(h_rx, d, len, hipMemcpyDeviceToHost, c->stream), HVWS_EHIP);
    }
    // one round trip for the results (the D2H of the bytes above is ordered before it)
    if ((rc = readback_all(c)) != HVWS_OK) return rc;
    if (carry) {
        for (uint32_t s = 0; s < nseg; ++s) {
            void* keep = carry[s].data;
            from_dcarry(c->hcarry[s], carry[s]);
            carry[s].data = keep;
        }
    }
    return HVWS_OK;
}

int hvws_pipeline(hvws_ctx* c, uint8_t* h_rx, uint64_t len, uint64_t chunk, websocket_parser* carry) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!carry) return set_err(HVWS_EINVAL, "carry required");
    if (chunk < 4096) chunk = 4096;
    chunk = (chunk + 15) & ~15ull;
    const uint64_t nchunks = (len + chunk - 1) / chunk;
    if (nchunks == 0) return HVWS_OK;
    // Three device slots: H2D(k+1) and D2H(k-1) overlap compute(k).  Slots
    // and events live in the context (grow-only), so repeated calls pay no
    // allocation; earlier work on the context's streams is finished first
    // (an earlier call's copies may still use the slots).
    HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);   // h_segs may still feed an earlier copy
    HIP_OR(hipStreamSynchronize(c->copy_in), HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(c->copy_out), HVWS_EHIP);
    dbuf* slot = c->pipe_slot;
    for (int i = 0; i < 3; ++i) HIP_OR(slot[i].ensure(chunk + 64), HVWS_ENOMEM);
    for (hipEvent_t& ev : c->pipe_ev)
        if (!ev) HIP_OR(hipEventCreateWithFlags(&ev, hipEventDisableTiming), HVWS_EHIP);
    hipEvent_t* in_done = c->pipe_ev;
    hipEvent_t* comp_done = c->pipe_ev + 3;
    hipEvent_t* out_done = c->pipe_ev + 6;
    // every chunk's segment {0, n}, resident before the loop
    dbuf& pipe_segs = c->pipe_segs;
    HIP_OR(pipe_segs.ensure(nchunks * sizeof(dseg)), HVWS_ENOMEM);
    HIP_OR(c->h_segs.ensure(nchunks * sizeof(dseg)), HVWS_ENOMEM);
    for (uint64_t k = 0; k < nchunks; ++k) c->h_segs.as<dseg>()[k] = dseg{0, std::min(chunk, len - k * chunk)};
    HIP_OR(hipMemcpyAsync(pipe_segs.p, c->h_segs.p, nchunks * sizeof(dseg), hipMemcpyHostToDevice, c->stream),
           HVWS_EHIP);
    hvws_segment seg0 = {0, 0};
    void* keep = carry->data;
    int out_rc = HVWS_OK;
    auto issue_in = [&](uint64_t k) -> hipError_t {
        const int s = (int)(k % 3);
        const uint64_t off = k * chunk;
        const uint64_t n = std::min(chunk, len - off);
        hipError_t e = hipStreamWaitEvent(c->copy_in, out_done[s], 0);
        if (e == hipSuccess) e = hipMemcpyAsync(slot[s].p, h_rx + off, n, hipMemcpyHostToDevice, c->copy_in);
        if (e == hipSuccess) e = hipEventRecord(in_done[s], c->copy_in);
        return e;
    };
    // out_done events start "complete"
    for (int i = 0; i < 3; ++i) hipEventRecord(out_done[i], c->copy_out);
    hipError_t e = issue_in(0);
    for (uint64_t k = 0; k < nchunks && e == hipSuccess && out_rc == HVWS_OK; ++k) {
        const int s = (int)(k % 3);
        const uint64_t off = k * chunk;
        const uint64_t n = std::min(chunk, len - off);
        if (k + 1 < nchunks) e = issue_in(k + 1);
        if (e != hipSuccess) break;
        e = hipStreamWaitEvent(c->stream, in_done[s], 0);
        if (e != hipSuccess) break;
        seg0.len = n;
        if (k == 0) {
            out_rc = upload_segments(c, &seg0, carry, 1, n);
        } else {
            // The carry chains on the device: chunk k-1's carry-out is chunk
            // k's carry-in (a frame may straddle the chunk boundary).
            // Both tables are copied device to device, so the host never
            // waits inside the loop (each chunk's segment is preloaded).
            e = hipMemcpyAsync(c->segs.p, pipe_segs.as<dseg>() + k, sizeof(dseg), hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(c->carry_in.p, c->T().carry_out.p, sizeof(dcarry), hipMemcpyDeviceToDevice,
                                   c->stream);
            if (e != hipSuccess) break;
        }
        if (out_rc != HVWS_OK) break;
        out_rc = scan_device_carry(c, slot[s].as<uint8_t>(), n, 1);
        if (out_rc != HVWS_OK) break;
        out_rc = hvws_unmask(c, slot[s].as<uint8_t>(), n);
        if (out_rc != HVWS_OK) break;
        e = hipEventRecord(comp_done[s], c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->copy_out, comp_done[s], 0);
        if (e == hipSuccess) e = hipMemcpyAsync(h_rx + off, slot[s].p, n, hipMemcpyDeviceToHost, c->copy_out);
        if (e == hipSuccess) e = hipEventRecord(out_done[s], c->copy_out);
    }
    if (e == hipSuccess && out_rc == HVWS_OK) {
        e = hipStreamSynchronize(c->copy_out);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) out_rc = hvws_get_carry(c, carry, nullptr);
    }
    hipStreamSynchronize(c->copy_in);
    hipStreamSynchronize(c->copy_out);
    hipStreamSynchronize(c->stream);
    carry->data = keep;
    // The last scan referenced a slot, which the next call overwrites:
    // forget it (hvws_unmask would refuse it anyway).
    c->have_scan = false;
    if (e != hipSuccess) return set_err(HVWS_EHIP, "pipeline: %s", hipGetErrorString(e));
    return out_rc;
}

// ------------------------------------------------------------------ synth
int hvws_synth(hvws_ctx* c, uint8_t* d_buf, uint64_t buf_len, uint64_t seed, uint64_t nframes,
               const uint64_t* d_frame_off, const uint8_t* d_flags, const uint32_t* d_mask,
               const uint64_t* d_length, const uint8_t* d_text, int mode, uint64_t* mismatches) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (mode < 0 || mode > 2) return set_err(HVWS_EINVAL, "bad synth mode %d", mode);
    const uint64_t tile = synth_tile();
    const uint64_t ntiles = (buf_len + tile - 1) / tile;
    HIP_OR(c->synth_sizes.ensure(nframes * 8 + 8), HVWS_ENOMEM);
    HIP_OR(c->synth_tiles.ensure((ntiles + 2) * 4), HVWS_ENOMEM);
    HIP_OR(c->synth_bad.ensure(8), HVWS_ENOMEM);
    HIP_OR(launch_frame_sizes(d_flags, d_length, nframes, c->synth_sizes.as<uint64_t>(), c->stream), HVWS_EHIP);
    HIP_OR(launch_tile_index(d_frame_off, c->synth_sizes.as<uint64_t>(), nframes, nullptr, c->synth_tiles.as<uint32_t>(),
                             ntiles, tile, c->stream),
           HVWS_EHIP);
    HIP_OR(hipMemsetAsync(c->synth_bad.p, 0, 8, c->stream), HVWS_EHIP);
    HIP_OR(launch_synth(d_buf, buf_len, seed, nframes, d_frame_off, d_flags, d_mask, d_length, d_text,
                        c->synth_sizes.as<uint64_t>(), c->synth_tiles.as<uint32_t>(), mode,
                        c->synth_bad.as<unsigned long long>(), c->stream),
           HVWS_EHIP);
    if (mode != HVWS_SYNTH_WRITE) {
        uint64_t bad = 0;
        HIP_OR(hipMemcpyAsync(&bad, c->synth_bad.p, 8, hipMemcpyDeviceToHost, c->stream), HVWS_EHIP);
        HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
        if (mismatches) *mismatches = bad;
    }
    return HVWS_OK;
}

int hvws_digest(hvws_ctx* c, const uint8_t* d_buf, uint64_t len, uint64_t* out) {
    int rc = check_ctx(c);
    if (rc) return rc;
    HIP_OR(c->synth_bad.ensure(8), HVWS_ENOMEM);
    HIP_OR(hipMemsetAsync(c->synth_bad.p, 0, 8, c->stream), HVWS_EHIP);
    HIP_OR(launch_digest(d_buf, len, c->synth_bad.as<unsigned long long>(), c->stream), HVWS_EHIP);
    uint64_t v = 0;
    HIP_OR(hipMemcpyAsync(&v, c->synth_bad.p, 8, hipMemcpyDeviceToHost, c->stream), HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    if (out) *out = v;
    return HVWS_OK;
}

// --------------------------------------------------------------- transmit
namespace {
int tx_build_checked(hvws_ctx* c, uint8_t* d_out, uint64_t total, const uint8_t* d_payload, uint64_t payload_len,
                     const uint64_t* d_pay_off, const uint64_t* d_len, const uint8_t* d_flags, const uint32_t* d_mask,
                     const uint64_t* off, const uint64_t* size, uint64_t n, const uint64_t* uh,
                     const std::function<hipError_t()>* pre);
}  // namespace

int hvws_build_frames(hvws_ctx* c, uint8_t* d_out, uint64_t out_cap, const uint8_t* d_payload, uint64_t payload_len,
                      const uint64_t* d_pay_off, const uint64_t* d_len, const uint8_t* d_flags, const uint32_t* d_mask,
                      uint64_t n, uint64_t* d_out_off, uint64_t* out_len) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (out_len) *out_len = 0;
    if (n == 0) return HVWS_OK;
    if (!d_out || !d_pay_off || !d_len || !d_flags) return set_err(HVWS_EINVAL, "build_frames: null table");
    if (n >= 0xFFFFFFFFull) return set_err(HVWS_EINVAL, "build_frames: %llu frames (max 2^32-2)", (unsigned long long)n);
    const uint64_t nb = (n + 1023) / 1024;
    HIP_OR(c->tx.size.ensure(n * 8 + 8), HVWS_ENOMEM);
    HIP_OR(c->tx.scan.ensure((4 * nb + 64) * 8), HVWS_ENOMEM);
    HIP_OR(c->tx.stat.ensure(64), HVWS_ENOMEM);
    HIP_OR(c->tx.h.ensure(64), HVWS_ENOMEM);
    uint64_t* off = d_out_off;
    if (!off) {
        HIP_OR(c->tx.off.ensure(n * 8 + 8), HVWS_ENOMEM);
        off = c->tx.off.as<uint64_t>();
    }
    // [0] total bytes, [1] payload ranges out of bounds, [2] frames breaking
    // the uniform layout, [3..5] pay_off[0], its step, len[0] (k_tx_check)
    uint64_t* stat = c->tx.stat.as<uint64_t>();
    HIP_OR(hipMemsetAsync(stat, 0, 64, c->stream), HVWS_EHIP);
    HIP_OR(launch_frame_sizes(d_flags, d_len, n, c->tx.size.as<uint64_t>(), c->stream), HVWS_EHIP);
    HIP_OR(launch_exclusive_scan(c->tx.size.as<uint64_t>(), off, n, c->tx.scan.as<uint64_t>(), stat, c->stream),
           HVWS_EHIP);
    HIP_OR(launch_tx_check(d_pay_off, d_len, d_flags, d_mask, c->tx.size.as<uint64_t>(), n, payload_len, stat,
                           c->stream),
           HVWS_EHIP);
    uint64_t* h = c->tx.h.as<uint64_t>();
    HIP_OR(hipMemcpyAsync(h, stat, 48, hipMemcpyDeviceToHost, c->stream), HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    if (h[1]) return set_err(HVWS_EINVAL, "build_frames: %llu frames read outside the payload buffer or lack a mask",
                             (unsigned long long)h[1]);
    const uint64_t total = h[0];
    if (out_len) *out_len = total;
    if (total > out_cap)
        return set_err(HVWS_EINVAL, "build_frames: output needs %llu bytes, capacity %llu", (unsigned long long)total,
                       (unsigned long long)out_cap);
    return tx_build_checked(c, d_out, total, d_payload, payload_len, d_pay_off, d_len, d_flags, d_mask, off,
                            c->tx.size.as<uint64_t>(), n, h + 2, nullptr);
}

namespace {
// The half of hvws_build_frames after its wait, shared with
// hvws_send_messages: n frames (rows d_pay_off .. size, total output bytes)
// whose tables the device has checked.  uh = {frames breaking the uniform
// layout, pay_off[0], its step, len[0]} (k_tx_check's stat[2..5]).  pre (may
// be null): device work queued inside the timed region ahead of the tile
// index (the send's expansion writes the rows there).
int tx_build_checked(hvws_ctx* c, uint8_t* d_out, uint64_t total, const uint8_t* d_payload, uint64_t payload_len,
                     const uint64_t* d_pay_off, const uint64_t* d_len, const uint8_t* d_flags, const uint32_t* d_mask,
                     const uint64_t* off, const uint64_t* size, uint64_t n, const uint64_t* uh,
                     const std::function<hipError_t()>* pre) {
    // the geometry by the batch's mean frame size (tx_variant); every layout
    // takes k_build (round 4: it reached or beat the same-offset kernel
    // k_build_id, which is gone, profiles/r4v_raw)
    const int v = tx_variant(total, n);
    c->tx.variant = v;
    // each tile's source span first (round 4: records-first tiles lost, and
    // their switch went in round 6)
    const bool spans_ok = true;
    const uint64_t tile = tx_tile(v);
    const uint64_t ntiles = (total + tile - 1) / tile;
    // A uniform layout (every frame the same size and length, payload offsets
    // a + k * b, b >= 0) needs no tile index: each tile finds its frames and
    // source span from its position.
    constexpr bool uni_ok = true;
    // (payload steps shorter than a payload would make a tile's pieces
    // overlap out of order: the index handles those)
    // (small frames only, the lean form: at 64 KiB frames the index is ~0.1 %
    // of the call and the position-derived form measured slower at the rx
    // layout, 21.3 against 20.2 ms at c3, profiles/r5b_raw)
    const bool uniform = uni_ok && v == 5 && uh[0] == 0 && total % n == 0 && (n == 1 || uh[2] >= uh[3]);
    const uint64_t uni[4] = {uniform ? total / n : 0, uniform ? total / n - uh[3] : 0, uh[1], uh[2]};
    c->tx.uniform = uniform;
    if (!uniform) {
        HIP_OR(c->tx.tiles.ensure((ntiles + 2) * 4), HVWS_ENOMEM);
        if (spans_ok) HIP_OR(c->tx.span.ensure(ntiles * 16 + 16), HVWS_ENOMEM);
    }
    // the timed device work (hvws_last_kernel_ms): tile index, spans, build
    HIP_OR(timed_begin(c), HVWS_EHIP);
    uint64_t* span = spans_ok && !uniform ? c->tx.span.as<uint64_t>() : nullptr;
    if (pre) HIP_OR((*pre)(), HVWS_EHIP);
    if (!uniform)
        HIP_OR(launch_tx_index(off, size, d_pay_off, d_len, d_flags, n, ntiles, tile, c->tx.tiles.as<uint32_t>(), span,
                               c->stream),
               HVWS_EHIP);
    HIP_OR(launch_build(d_out, total, d_payload, payload_len, d_pay_off, d_len, d_flags, d_mask, off, size,
                        c->tx.tiles.as<uint32_t>(), span, n, v, c->stream, uni),
           HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    return HVWS_OK;
}
}  // namespace

static_assert(sizeof(dtxmsg) == sizeof(hvws_tx_msg) && sizeof(dtxmsg) == 24, "dtxmsg mirrors hvws_tx_msg");
static_assert(R_PONG == HVWS_R_PONG && R_CLOSE == HVWS_R_CLOSE && R_ECHO == HVWS_R_ECHO &&
                  RF_CLOSED == HVWS_RF_CLOSED && RF_DEFERRED == HVWS_RF_DEFERRED,
              "reply policy and flag bits");

// WebSocketChannel::send for a batch (hvws_send.hip): the message pass, one
// wait for {frames, bytes, bad}, then the expansion into per-frame rows and
// hvws_build_frames' own index and k_build.
int hvws_send_messages(hvws_ctx* c, uint8_t* d_out, uint64_t out_cap, const uint8_t* d_payload, uint64_t payload_len,
                       const hvws_tx_msg* d_msgs, uint64_t n, const uint64_t* d_n, uint64_t fragment, int masked,
                       uint64_t* d_msg_off, uint64_t* out_len, uint64_t* out_frames) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (out_len) *out_len = 0;
    if (out_frames) *out_frames = 0;
    if (n == 0) {
        if (d_msg_off) HIP_OR(hipMemsetAsync(d_msg_off, 0, 8, c->stream), HVWS_EHIP);
        return HVWS_OK;
    }
    if (!d_out || !d_msgs || (!d_payload && payload_len)) return set_err(HVWS_EINVAL, "send_messages: null table");
    if (((uintptr_t)d_out & 15u) != 0) return set_err(HVWS_EINVAL, "send_messages: d_out must be 16-byte aligned");
    {
        const uintptr_t o = (uintptr_t)d_out, p = (uintptr_t)d_payload;
        if (o < p + payload_len && p < o + out_cap)
            return set_err(HVWS_EINVAL, "send_messages: d_out overlaps the payload buffer");
    }
    // every message has a frame
    if (n >= 0xFFFFFFFFull) return set_err(HVWS_EINVAL, "send_messages: %llu messages (max 2^32-2)", (unsigned long long)n);
    const uint64_t F = fragment ? fragment : 0xFFFFu;   // WebSocketChannel.cpp:6
    const dtxmsg* msgs = reinterpret_cast<const dtxmsg*>(d_msgs);
    HIP_OR(c->sd.scan.ensure(send_scratch_bytes(n)), HVWS_ENOMEM);
    HIP_OR(c->sd.first.ensure(n * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->sd.meta.ensure(64), HVWS_ENOMEM);
    HIP_OR(c->tx.h.ensure(64), HVWS_ENOMEM);
    uint64_t* meta = c->sd.meta.as<uint64_t>();
    HIP_OR(hipMemsetAsync(meta, 0, 64, c->stream), HVWS_EHIP);
    HIP_OR(launch_send_table(msgs, n, d_n, payload_len, F, masked, c->sd.scan.p, c->sd.first.as<uint64_t>(), d_msg_off,
                             meta, c->stream),
           HVWS_EHIP);
    // [0] frames, [1] bytes, [2] bad messages, [3] effective count, [4] messages
    // breaking the uniform layout, [5..7] off[0], its step, len[0]
    uint64_t* h = c->tx.h.as<uint64_t>();
    HIP_OR(hipMemcpyAsync(h, meta, 64, hipMemcpyDeviceToHost, c->stream), HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(c->stream), HVWS_EHIP);
    if (h[2])
        return set_err(HVWS_EINVAL, "send_messages: %llu messages lie outside the payload buffer or have a flag bit "
                       "outside 0x1F", (unsigned long long)h[2]);
    const uint64_t nfr = h[0], total = h[1];
    if (out_len) *out_len = total;
    if (nfr > 0xFFFFFFFEull)
        return set_err(HVWS_EINVAL, "send_messages: %llu frames (max 2^32-2)", (unsigned long long)nfr);
    if (total > out_cap)
        return set_err(HVWS_EINVAL, "send_messages: output needs %llu bytes, capacity %llu", (unsigned long long)total,
                       (unsigned long long)out_cap);
    if (out_frames) *out_frames = nfr;
    if (nfr == 0) {   // *d_n was 0: nothing to build; the timed region is empty
        HIP_OR(timed_begin(c), HVWS_EHIP);
        HIP_OR(timed_end(c), HVWS_EHIP);
        return HVWS_OK;
    }
    HIP_OR(c->sd.poff.ensure(nfr * 8 + 8), HVWS_ENOMEM);
    HIP_OR(c->sd.len.ensure(nfr * 8 + 8), HVWS_ENOMEM);
    HIP_OR(c->sd.flags.ensure(nfr + 8), HVWS_ENOMEM);
    HIP_OR(c->sd.mask.ensure(nfr * 4 + 8), HVWS_ENOMEM);
    HIP_OR(c->tx.off.ensure(nfr * 8 + 8), HVWS_ENOMEM);
    HIP_OR(c->tx.size.ensure(nfr * 8 + 8), HVWS_ENOMEM);
    const std::function<hipError_t()> expand = [&]() {
        return launch_send_expand(msgs, c->sd.scan.p, c->sd.first.as<uint64_t>(), meta, nfr, F, masked,
                                  c->sd.poff.as<uint64_t>(), c->sd.len.as<uint64_t>(), c->sd.flags.as<uint8_t>(),
                                  c->sd.mask.as<uint32_t>(), c->tx.off.as<uint64_t>(), c->tx.size.as<uint64_t>(),
                                  c->stream);
    };
    // the frames form a uniform layout when the messages do, one frame each
    const uint64_t uh[4] = {h[4] + (nfr != h[3] ? 1u : 0u), h[5], h[6], h[7]};
    return tx_build_checked(c, d_out, total, d_payload, payload_len, c->sd.poff.as<uint64_t>(),
                            c->sd.len.as<uint64_t>(), c->sd.flags.as<uint8_t>(), c->sd.mask.as<uint32_t>(),
                            c->tx.off.as<uint64_t>(), c->tx.size.as<uint64_t>(), nfr, uh, &expand);
}

// The server's onMessage dispatch over the last hvws_messages' pieces
// (hvws_send.hip): no wait.
namespace {
int replies_pass(hvws_ctx* c, uint32_t policy, const uint8_t* closed_in, bool checked) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!c->mg.have) return set_err(HVWS_EINVAL, "hvws_replies without a preceding hvws_messages");
    if (checked && (!c->mg.rfc || !c->ck.have || c->ck.msg != c->mg.seq))
        return set_err(HVWS_EINVAL, "hvws_replies_checked without an hvws_check of the last hvws_messages_rfc");
    if (policy & ~(uint32_t)(HVWS_R_PONG | HVWS_R_CLOSE | HVWS_R_ECHO))
        return set_err(HVWS_EINVAL, "hvws_replies: unknown policy bits");
    const uint32_t nseg = c->mg.nseg;
    const uint64_t cap = c->mg.cap;
    HIP_OR(c->rp.scan.ensure(rep_scratch_words(cap) * 8), HVWS_ENOMEM);
    HIP_OR(c->rp.limit.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->rp.msgs.ensure((cap + 1) * sizeof(dtxmsg)), HVWS_ENOMEM);
    HIP_OR(c->rp.piece.ensure((cap + 1) * 8), HVWS_ENOMEM);
    HIP_OR(c->rp.first.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->rp.count.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->rp.flags.ensure((uint64_t)nseg + 16), HVWS_ENOMEM);
    HIP_OR(c->rp.closed.ensure((uint64_t)nseg + 16), HVWS_ENOMEM);
    c->rp.have = false;   // the tables are being rewritten
    if ((rc = c->rp.up.send(c->rp.closed.p, c->stream, closed_in, nseg)) != HVWS_OK) return rc;
    HIP_OR(launch_replies(c->mg.msgs.as<dmsg>(), c->mg.meta.as<uint64_t>(), cap, c->mg.first.as<uint64_t>(),
                          c->mg.count.as<uint64_t>(), nseg, policy, closed_in ? c->rp.closed.as<uint8_t>() : nullptr,
                          c->rp.limit.as<uint64_t>(), c->rp.scan.as<uint64_t>(), c->rp.msgs.as<dtxmsg>(),
                          c->rp.piece.as<uint64_t>(), c->rp.first.as<uint64_t>(), c->rp.count.as<uint64_t>(),
                          c->rp.flags.as<uint8_t>(), c->mg.rfc, c->stream,
                          checked ? c->ck.fail.as<uint64_t>() : nullptr),
           HVWS_EHIP);
    c->rp.have = true;
    c->rp.nseg = nseg;
    c->rp.cap = cap;
    c->rp.gen = c->scan_gen;
    ++c->rp.seq;
    return HVWS_OK;
}
}  // namespace

int hvws_replies(hvws_ctx* c, uint32_t policy, const uint8_t* closed_in) {
    return replies_pass(c, policy, closed_in, false);
}

// hvws_replies with hvws_check's fail_rec as a second per-connection limit.
int hvws_replies_checked(hvws_ctx* c, uint32_t policy, const uint8_t* closed_in) {
    return replies_pass(c, policy, closed_in, true);
}

static_assert(CK_HEADER == HVWS_C_HEADER && CK_SEQUENCE == HVWS_C_SEQUENCE && CK_CLOSE_BODY == HVWS_C_CLOSE_BODY &&
                  CK_CLOSE_UTF8 == HVWS_C_CLOSE_UTF8 && CK_TEXT_UTF8 == HVWS_C_TEXT_UTF8 && CK_SIZE == HVWS_C_SIZE &&
                  CK_ALL == HVWS_C_ALL && CK_OPEN == HVWS_CK_OPEN && CK_FAILED == HVWS_CK_FAILED &&
                  RF_FAILED == HVWS_RF_FAILED,
              "check bits");

// Which connections of the last hvws_messages_rfc must be failed, where and
// why (hvws_check.hip): asynchronous on the context stream, no wait.
int hvws_check(hvws_ctx* c, uint32_t classes, uint64_t max_message, const uint32_t* state_in) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!c->mg.have || !c->mg.rfc) return set_err(HVWS_EINVAL, "hvws_check without a preceding hvws_messages_rfc");
    if (c->mg.gen != c->scan_gen) return set_err(HVWS_EINVAL, "hvws_check: a scan has run since hvws_messages_rfc");
    if (classes & ~(uint32_t)HVWS_C_ALL) return set_err(HVWS_EINVAL, "hvws_check: unknown class bits");
    const uint32_t nseg = c->mg.nseg;
    if ((classes & HVWS_C_TEXT_UTF8) && (!c->u8.have || c->u8.gen != c->scan_gen || c->u8.nseg != nseg))
        return set_err(HVWS_EINVAL, "hvws_check: HVWS_C_TEXT_UTF8 without an hvws_utf8 over the same scan");
    if (state_in)
        for (uint32_t s = 0; s < nseg; ++s)
            if (state_in[s] & ~(uint32_t)(HVWS_CK_OPEN | HVWS_CK_FAILED))
                return set_err(HVWS_EINVAL, "hvws_check: state_in is no state hvws_get_check returns");
    // the record bound hvws_messages_rfc ran with, or the count read since
    const uint64_t cap = record_bound(c);
    const uint64_t pcap = c->mg.cap;
    HIP_OR(c->ck.scan.ensure(check_scratch_bytes(cap)), HVWS_ENOMEM);
    HIP_OR(c->ck.viol.ensure(cap + pcap + 16), HVWS_ENOMEM);
    HIP_OR(c->ck.in.ensure((uint64_t)nseg * 4 + 16), HVWS_ENOMEM);
    HIP_OR(c->ck.out.ensure((uint64_t)nseg * 4 + 16), HVWS_ENOMEM);
    HIP_OR(c->ck.fail.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->ck.why.ensure((uint64_t)nseg * 4 + 16), HVWS_ENOMEM);
    HIP_OR(c->ck.code.ensure((uint64_t)nseg * 2 + 16), HVWS_ENOMEM);
    c->ck.have = false;   // the tables are being rewritten
    if ((rc = c->ck.up.send(c->ck.in.p, c->stream, state_in, (uint64_t)nseg * 4)) != HVWS_OK) return rc;
    HIP_OR(timed_begin(c), HVWS_EHIP);
    HIP_OR(launch_check(c->T().f_info.as<uint32_t>(), c->T().f_length.as<uint64_t>(), c->T().total.as<uint64_t>(), cap,
                        c->T().bases.as<uint64_t>(), nseg, c->mg.msgs.as<dmsg>(), c->mg.meta.as<uint64_t>(), pcap,
                        c->mg.dout, c->mg.out_cap, c->u8.bad.as<uint64_t>(), classes, max_message,
                        state_in ? c->ck.in.as<uint32_t>() : nullptr, c->ck.scan.p, c->ck.viol.as<uint8_t>(),
                        c->ck.out.as<uint32_t>(), c->ck.fail.as<uint64_t>(), c->ck.why.as<uint32_t>(),
                        c->ck.code.as<uint16_t>(), c->stream),
           HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    HIP_OR(hold_tables(c), HVWS_EHIP);
    c->ck.have = true;
    c->ck.nseg = nseg;
    c->ck.msg = c->mg.seq;
    return HVWS_OK;
}

int hvws_get_check(hvws_ctx* c, uint32_t* state_out, uint64_t* fail_rec, uint32_t* why, uint16_t* code) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->ck.have) return set_err(HVWS_EINVAL, "no hvws_check call yet");
    const uint64_t nseg = c->ck.nseg;
    return read_rows(c, {{state_out, c->ck.out.p, nseg * 4},
                         {fail_rec, c->ck.fail.p, nseg * 8},
                         {why, c->ck.why.p, nseg * 4},
                         {code, c->ck.code.p, nseg * 2}});
}

const uint64_t* hvws_check_device(hvws_ctx* c) {
    if (!c || !c->ck.have) return nullptr;
    return c->ck.fail.as<uint64_t>();
}

const hvws_tx_msg* hvws_replies_device(hvws_ctx* c) {
    if (!c || !c->rp.have) return nullptr;
    return c->rp.msgs.as<hvws_tx_msg>();
}

const uint64_t* hvws_reply_count_device(hvws_ctx* c) {
    if (!c || !c->rp.have) return nullptr;
    return c->rp.scan.as<uint64_t>() + c->rp.cap;
}

uint64_t hvws_reply_capacity(hvws_ctx* c) { return c && c->rp.have ? c->rp.cap : 0; }

int64_t hvws_reply_count(hvws_ctx* c) {
    if (check_ctx(c)) return -1;
    if (!c->rp.have) {
        set_err(HVWS_EINVAL, "no hvws_replies call yet");
        return -1;
    }
    return read_count(c, c->rp.scan.as<uint64_t>() + c->rp.cap, "hvws_reply_count");
}

int hvws_get_replies(hvws_ctx* c, hvws_tx_msg* out, uint64_t* piece, uint64_t first, uint64_t n) {
    const int64_t have = hvws_reply_count(c);
    if (have < 0) return HVWS_EINVAL;
    if (first > (uint64_t)have || n > (uint64_t)have - first) return set_err(HVWS_EINVAL, "reply range out of bounds");
    if (n == 0) return HVWS_OK;
    return read_rows(c, {{out, c->rp.msgs.as<dtxmsg>() + first, n * sizeof(dtxmsg)},
                         {piece, c->rp.piece.as<uint64_t>() + first, n * 8}});
}

int hvws_get_segment_replies(hvws_ctx* c, uint64_t* first, uint64_t* count) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->rp.have) return set_err(HVWS_EINVAL, "no hvws_replies call yet");
    const uint64_t nseg = c->rp.nseg;
    return read_rows(c, {{first, c->rp.first.p, nseg * 8}, {count, c->rp.count.p, nseg * 8}});
}

int hvws_get_reply_flags(hvws_ctx* c, uint8_t* out) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->rp.have) return set_err(HVWS_EINVAL, "no hvws_replies call yet");
    return read_rows(c, {{out, c->rp.flags.p, c->rp.nseg}});
}

static_assert(HVWS_FAN_NONE == 0xFFFFFFFFu && HVWS_FAN_SELF == 1u, "fanout constants");

namespace {
int fan_run(hvws_ctx* c, const char* who, const fan_tables& t, uint64_t per, uint64_t max_deliveries,
            uint64_t* out_deliveries);
}

// The last reply call's table through a subscription table, ordered by
// destination (hvws_fan.hip): the edge count, one wait for {edges, deliveries,
// bad}, then expansion, sort and finish.
int hvws_fanout(hvws_ctx* c, const uint64_t* d_topic_first, const uint32_t* d_member, uint32_t ntopics,
                uint64_t nmember, uint32_t ndest, const uint32_t* pub, const uint32_t* dest_of, uint32_t flags,
                uint64_t max_deliveries, uint64_t* out_deliveries) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (out_deliveries) *out_deliveries = 0;
    c->fan.have = false;   // the tables are being rewritten
    c->bg.have = false;    // ... which a budget pass ran over
    if (!c->rp.have || !c->mg.have) return set_err(HVWS_EINVAL, "hvws_fanout without a preceding hvws_replies");
    if (c->rp.gen != c->scan_gen) return set_err(HVWS_EINVAL, "hvws_fanout: a scan has run since hvws_replies");
    if (flags & ~(uint32_t)HVWS_FAN_SELF) return set_err(HVWS_EINVAL, "hvws_fanout: unknown flag bits");
    if (!dest_of) return set_err(HVWS_EINVAL, "hvws_fanout: null dest_of");
    if (ndest == 0 || ndest > 0x7FFFFFFFu)
        return set_err(HVWS_EINVAL, "hvws_fanout: %u destinations (1 .. 2^31-1)", ndest);
    const uint32_t nseg = c->rp.nseg;
    bool publishes = false;
    for (uint32_t s = 0; s < nseg; ++s) {
        if (dest_of[s] >= ndest)
            return set_err(HVWS_EINVAL, "hvws_fanout: dest_of[%u] = %u of %u destinations", s, dest_of[s], ndest);
        if (pub && pub[s] != HVWS_FAN_NONE) {
            if (pub[s] >= ntopics)
                return set_err(HVWS_EINVAL, "hvws_fanout: pub[%u] = %u of %u topics", s, pub[s], ntopics);
            publishes = true;
        }
    }
    if (publishes && (!d_topic_first || (!d_member && nmember)))
        return set_err(HVWS_EINVAL, "hvws_fanout: null subscription table");
    const uint64_t cap = c->rp.cap;
    // every reply and every edge has a 32-bit index
    if (cap >= 0xFFFFFFFFull) return set_err(HVWS_EINVAL, "hvws_fanout: %llu replies (max 2^32-2)", (unsigned long long)cap);
    HIP_OR(c->fan.in.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    // dest_of, then pub behind it
    if ((rc = c->fan.up.send(c->fan.in.p, c->stream, dest_of, (uint64_t)nseg * 4, publishes ? pub : nullptr,
                             publishes ? (uint64_t)nseg * 4 : 0)) != HVWS_OK)
        return rc;
    const fan_tables t{c->rp.msgs.as<dtxmsg>(), c->rp.piece.as<uint64_t>(), c->rp.scan.as<uint64_t>() + cap, cap,
                       c->mg.msgs.as<dmsg>(), c->mg.meta.as<uint64_t>(), c->mg.cap, nseg, c->fan.in.as<uint32_t>(),
                       publishes ? c->fan.in.as<uint32_t>() + nseg : nullptr, d_topic_first, d_member, ntopics, nmember,
                       ndest, (flags & HVWS_FAN_SELF) != 0};
    return fan_run(c, "hvws_fanout", t, nseg, max_deliveries, out_deliveries);
}

namespace {
// What hvws_fanout and hvws_fanout_routed share once their tables stand: the
// edge count, the one wait, then expansion, sort and finish.  per: the self
// counts and bad marks the count keeps (one per segment; routed: per reply).
int fan_run(hvws_ctx* c, const char* who, const fan_tables& t, uint64_t per, uint64_t max_deliveries,
            uint64_t* out_deliveries) {
    int rc;
    const uint32_t ndest = t.ndest;
    HIP_OR(c->fan.scan.ensure(fan_scratch_bytes(t.rep_cap)), HVWS_ENOMEM);
    HIP_OR(c->fan.seg.ensure(per * 16 + 16), HVWS_ENOMEM);
    HIP_OR(c->fan.meta.ensure(64), HVWS_ENOMEM);
    uint64_t* selfc = c->fan.seg.as<uint64_t>();
    uint32_t* mark = reinterpret_cast<uint32_t*>(selfc + per);
    uint64_t* meta = c->fan.meta.as<uint64_t>();
    HIP_OR(launch_fan_count(t, mark, selfc, mark + per, c->fan.scan.p, meta, c->stream), HVWS_EHIP);
    // the one wait: [0] edges before the self drop, [1] deliveries, [2] bad replies, [3] replies
    uint64_t h[4] = {0, 0, 0, 0};
    if ((rc = read_rows(c, {{h, meta, sizeof h}})) != HVWS_OK) return rc;
    const uint64_t nedges = h[0], ndel = h[1];
    if (out_deliveries) *out_deliveries = ndel;
    if (h[2])
        return set_err(HVWS_EINVAL, "%s: %llu publications reach a topic row outside the member table or a "
                       "member id outside the destinations", who, (unsigned long long)h[2]);
    if (ndel > max_deliveries)
        return set_err(HVWS_EINVAL, "%s: %llu deliveries, max_deliveries %llu", who, (unsigned long long)ndel,
                       (unsigned long long)max_deliveries);
    if (nedges > 0xFFFFFFFEull)
        return set_err(HVWS_EINVAL, "%s: %llu edges (max 2^32-2)", who, (unsigned long long)nedges);
    HIP_OR(c->fan.ping.ensure(nedges * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->fan.pong.ensure(nedges * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->fan.hist.ensure(fan_hist_words(nedges) * 8), HVWS_ENOMEM);
    HIP_OR(c->fan.msgs.ensure((ndel + 1) * sizeof(dtxmsg)), HVWS_ENOMEM);
    HIP_OR(c->fan.reply.ensure((ndel + 1) * 8), HVWS_ENOMEM);
    HIP_OR(c->fan.first.ensure((uint64_t)ndest * 8 + 16), HVWS_ENOMEM);
    HIP_OR(c->fan.count.ensure((uint64_t)ndest * 8 + 16), HVWS_ENOMEM);
    uint32_t* key[2] = {c->fan.ping.as<uint32_t>(), c->fan.pong.as<uint32_t>()};
    uint32_t* val[2] = {key[0] + nedges, key[1] + nedges};
    // the timed device work (hvws_last_kernel_ms): expansion, sort, finish
    HIP_OR(timed_begin(c), HVWS_EHIP);
    HIP_OR(launch_fan_deliver(t, c->fan.scan.p, nedges, ndel, key, val, c->fan.hist.as<uint64_t>(),
                              c->fan.msgs.as<dtxmsg>(), c->fan.reply.as<uint64_t>(), c->fan.first.as<uint64_t>(),
                              c->fan.count.as<uint64_t>(), &c->fan.key_in, c->stream),
           HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    c->fan.have = true;
    c->fan.ndest = ndest;
    c->fan.n = ndel;
    c->fan.rep = c->rp.seq;
    c->fan.msg = c->mg.seq;
    c->fan.maxlen = c->mg.out_cap;   // the rows point into the message call's output
    return HVWS_OK;
}

// The last hvws_fanout's tables stand: no reply or message call since.
bool fan_valid(const hvws_ctx* c) {
    return c && c->fan.have && c->rp.have && c->fan.rep == c->rp.seq && c->fan.msg == c->mg.seq;
}
}  // namespace

const hvws_tx_msg* hvws_fanout_device(hvws_ctx* c) { return fan_valid(c) ? c->fan.msgs.as<hvws_tx_msg>() : nullptr; }

const uint64_t* hvws_fanout_count_device(hvws_ctx* c) { return fan_valid(c) ? c->fan.meta.as<uint64_t>() + 1 : nullptr; }

int64_t hvws_fanout_count(hvws_ctx* c) {
    if (check_ctx(c)) return -1;
    if (!fan_valid(c)) {
        set_err(HVWS_EINVAL, "no hvws_fanout call yet");
        return -1;
    }
    return (int64_t)c->fan.n;
}

int hvws_get_fanout(hvws_ctx* c, hvws_tx_msg* out, uint64_t* reply, uint64_t first, uint64_t n) {
    const int64_t have = hvws_fanout_count(c);
    if (have < 0) return HVWS_EINVAL;
    if (first > (uint64_t)have || n > (uint64_t)have - first) return set_err(HVWS_EINVAL, "delivery range out of bounds");
    if (n == 0) return HVWS_OK;
    return read_rows(c, {{out, c->fan.msgs.as<dtxmsg>() + first, n * sizeof(dtxmsg)},
                         {reply, c->fan.reply.as<uint64_t>() + first, n * 8}});
}

int hvws_get_dest_fanout(hvws_ctx* c, uint64_t* first, uint64_t* count) {
    if (int rc = check_ctx(c)) return rc;
    if (!fan_valid(c)) return set_err(HVWS_EINVAL, "no hvws_fanout call yet");
    const uint64_t nd = c->fan.ndest;
    return read_rows(c, {{first, c->fan.first.p, nd * 8}, {count, c->fan.count.p, nd * 8}});
}

static_assert(RK_OTHER == HVWS_RK_OTHER && RK_PUB == HVWS_RK_PUB && RK_SUB == HVWS_RK_SUB && RK_UNSUB == HVWS_RK_UNSUB &&
                  RK_BAD == HVWS_RK_BAD && RK_STOPPED == HVWS_RK_STOPPED && RT_BAD == HVWS_RT_BAD &&
                  HVWS_ROUTE_HDR_MAX == 12 && HVWS_ROUTE_NONE == ~0ull,
              "route constants");

// The last reply call's TEXT / BINARY replies classified by their command
// header (hvws_route.hip): the parse, one scan, the finish.  No wait.
int hvws_route(hvws_ctx* c, uint32_t ntopics, uint32_t ndest, const uint32_t* dest_of) {
    int rc = check_ctx(c);
    if (rc) return rc;
    pass_route& p = c->rt;
    p.have = false;   // the tables are being rewritten
    ++p.seq;
    if (!c->rp.have || !c->mg.have) return set_err(HVWS_EINVAL, "hvws_route without a preceding hvws_replies");
    if (c->rp.gen != c->scan_gen) return set_err(HVWS_EINVAL, "hvws_route: a scan has run since hvws_replies");
    if (!dest_of) return set_err(HVWS_EINVAL, "hvws_route: null dest_of");
    if (ndest == 0 || ndest > 0x7FFFFFFFu) return set_err(HVWS_EINVAL, "hvws_route: %u destinations (1 .. 2^31-1)", ndest);
    const uint32_t nseg = c->rp.nseg;
    for (uint32_t s = 0; s < nseg; ++s)
        if (dest_of[s] >= ndest)
            return set_err(HVWS_EINVAL, "hvws_route: dest_of[%u] = %u of %u destinations", s, dest_of[s], ndest);
    const uint64_t cap = c->rp.cap;
    // every reply has a 32-bit index
    if (cap >= 0xFFFFFFFFull) return set_err(HVWS_EINVAL, "hvws_route: %llu replies (max 2^32-2)", (unsigned long long)cap);
    HIP_OR(p.scan.ensure(route_scratch_bytes(cap)), HVWS_ENOMEM);
    HIP_OR(p.in.ensure((uint64_t)nseg * 4 + 16), HVWS_ENOMEM);
    HIP_OR(p.rows.ensure((cap + 1) * sizeof(dtxmsg)), HVWS_ENOMEM);
    HIP_OR(p.topic.ensure((cap + 1) * 4), HVWS_ENOMEM);
    HIP_OR(p.kind.ensure(cap + 16), HVWS_ENOMEM);
    HIP_OR(p.bad.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.flags.ensure((uint64_t)nseg + 16), HVWS_ENOMEM);
    HIP_OR(p.ev.ensure((cap + 1) * sizeof(dsubev)), HVWS_ENOMEM);
    HIP_OR(p.meta.ensure(64), HVWS_ENOMEM);
    if ((rc = p.up.send(p.in.p, c->stream, dest_of, (uint64_t)nseg * 4)) != HVWS_OK) return rc;
    const route_tables t{c->rp.msgs.as<dtxmsg>(), c->rp.piece.as<uint64_t>(), c->rp.scan.as<uint64_t>() + cap, cap,
                         c->mg.msgs.as<dmsg>(), c->mg.meta.as<uint64_t>(), c->mg.cap, nseg, p.in.as<uint32_t>(), ntopics,
                         c->mg.dout, c->mg.dout ? c->mg.out_cap : 0};
    const route_work w{p.rows.as<dtxmsg>(), p.topic.as<uint32_t>(), p.kind.as<uint8_t>(), p.bad.as<uint64_t>(),
                       p.flags.as<uint8_t>(), p.ev.as<dsubev>(), p.scan.p, p.meta.as<uint64_t>()};
    // the timed device work (hvws_last_kernel_ms): the whole pass
    HIP_OR(timed_begin(c), HVWS_EHIP);
    HIP_OR(launch_route(t, w, c->stream), HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    p.have = true;
    p.nseg = nseg;
    p.ntopics = ntopics;
    p.ndest = ndest;
    p.rep = c->rp.seq;
    p.msg = c->mg.seq;
    p.gen = c->scan_gen;
    return HVWS_OK;
}

namespace {
// The last hvws_route's tables stand: no reply call, message call or scan since.
bool route_valid(const hvws_ctx* c) {
    return c && c->rt.have && c->rp.have && c->rt.rep == c->rp.seq && c->rt.msg == c->mg.seq && c->rt.gen == c->scan_gen;
}
int route_ctx(hvws_ctx* c) {
    if (int rc = check_ctx(c)) return rc;
    return route_valid(c) ? HVWS_OK : set_err(HVWS_EINVAL, "no hvws_route call yet");
}
}  // namespace

const hvws_tx_msg* hvws_route_device(hvws_ctx* c) { return route_valid(c) ? c->rt.rows.as<hvws_tx_msg>() : nullptr; }

const uint32_t* hvws_route_topics_device(hvws_ctx* c) { return route_valid(c) ? c->rt.topic.as<uint32_t>() : nullptr; }

const hvws_sub_event* hvws_route_events_device(hvws_ctx* c) {
    return route_valid(c) ? c->rt.ev.as<hvws_sub_event>() : nullptr;
}

const uint64_t* hvws_route_event_count_device(hvws_ctx* c) { return route_valid(c) ? c->rt.meta.as<uint64_t>() : nullptr; }

int hvws_get_route(hvws_ctx* c, hvws_tx_msg* rows, uint32_t* topic, uint8_t* kind, uint64_t first, uint64_t n) {
    if (int rc = route_ctx(c)) return rc;
    const int64_t have = hvws_reply_count(c);
    if (have < 0) return HVWS_EINVAL;
    if (first > (uint64_t)have || n > (uint64_t)have - first) return set_err(HVWS_EINVAL, "reply range out of bounds");
    if (n == 0) return HVWS_OK;
    return read_rows(c, {{rows, c->rt.rows.as<dtxmsg>() + first, n * sizeof(dtxmsg)},
                         {topic, c->rt.topic.as<uint32_t>() + first, n * 4},
                         {kind, c->rt.kind.as<uint8_t>() + first, n}});
}

int64_t hvws_route_event_count(hvws_ctx* c) {
    if (route_ctx(c)) return -1;
    return read_count(c, c->rt.meta.as<uint64_t>(), "hvws_route_event_count");
}

int hvws_get_route_events(hvws_ctx* c, hvws_sub_event* out, uint64_t first, uint64_t n) {
    const int64_t have = hvws_route_event_count(c);
    if (have < 0) return HVWS_EINVAL;
    if (first > (uint64_t)have || n > (uint64_t)have - first) return set_err(HVWS_EINVAL, "event range out of bounds");
    if (n == 0) return HVWS_OK;
    return read_rows(c, {{out, c->rt.ev.as<dsubev>() + first, n * sizeof(dsubev)}});
}

int hvws_get_route_flags(hvws_ctx* c, uint8_t* flags, uint64_t* bad_reply) {
    if (int rc = route_ctx(c)) return rc;
    const uint64_t nseg = c->rt.nseg;
    return read_rows(c, {{flags, c->rt.flags.p, nseg}, {bad_reply, c->rt.bad.p, nseg * 8}});
}

int hvws_get_route_totals(hvws_ctx* c, uint64_t out[4]) {
    if (int rc = route_ctx(c)) return rc;
    if (!out) return set_err(HVWS_EINVAL, "hvws_get_route_totals: null out");
    return read_rows(c, {{out, c->rt.meta.as<uint64_t>() + 1, 32}});
}

// hvws_fanout with the topic per reply and the rows of the last hvws_route.
int hvws_fanout_routed(hvws_ctx* c, const uint64_t* d_topic_first, const uint32_t* d_member, uint64_t nmember,
                       uint32_t flags, uint64_t max_deliveries, uint64_t* out_deliveries) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (out_deliveries) *out_deliveries = 0;
    c->fan.have = false;   // the tables are being rewritten
    c->bg.have = false;    // ... which a budget pass ran over
    if (!route_valid(c)) return set_err(HVWS_EINVAL, "hvws_fanout_routed without a preceding hvws_route");
    if (flags & ~(uint32_t)HVWS_FAN_SELF) return set_err(HVWS_EINVAL, "hvws_fanout_routed: unknown flag bits");
    // which replies publish is known on the device alone: with a topic to publish to, the table must be there
    if (c->rt.ntopics && (!d_topic_first || (!d_member && nmember)))
        return set_err(HVWS_EINVAL, "hvws_fanout_routed: null subscription table");
    const uint64_t cap = c->rp.cap;   // < 2^32 - 1: hvws_route saw it
    const fan_tables t{c->rt.rows.as<dtxmsg>(), c->rp.piece.as<uint64_t>(), c->rp.scan.as<uint64_t>() + cap, cap,
                       c->mg.msgs.as<dmsg>(), c->mg.meta.as<uint64_t>(), c->mg.cap, c->rt.nseg, c->rt.in.as<uint32_t>(),
                       nullptr, d_topic_first, d_member, c->rt.ntopics, nmember, c->rt.ndest,
                       (flags & HVWS_FAN_SELF) != 0, c->rt.topic.as<uint32_t>()};
    return fan_run(c, "hvws_fanout_routed", t, cap, max_deliveries, out_deliveries);
}

static_assert(sizeof(dretained) == sizeof(hvws_retained) && sizeof(dretained) == 16, "dretained mirrors hvws_retained");

namespace {
// [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na && nb && x < y + nb && y < x + na;
}
}  // namespace

namespace {
// What hvws_retain and hvws_retain_enveloped share once the route (and the
// envelope) is known to stand: rows / src[0, src_cap) are the winners' rows and
// the buffer they point into; the message call's output may not overlap the
// store either way.
int retain_run(hvws_ctx* c, const char* who, const dtxmsg* rows, const uint8_t* src, uint64_t src_cap, uint8_t* d_store,
               uint64_t slot, hvws_retained* d_ret) {
    pass_retain& p = c->rn;
    if (slot == 0 || (slot & 15u)) return set_err(HVWS_EINVAL, "%s: slot = %llu (a multiple of 16, not 0)", who,
                                                  (unsigned long long)slot);
    const uint32_t ntopics = c->rt.ntopics, nseg = c->rt.nseg;
    if (ntopics && slot > ~0ull / ntopics)
        return set_err(HVWS_EINVAL, "%s: %u slots of %llu bytes exceed 64 bits", who, ntopics, (unsigned long long)slot);
    const uint64_t store_len = (uint64_t)ntopics * slot, ret_len = (uint64_t)ntopics * sizeof(dretained);
    const uint8_t* dout = c->mg.dout;
    const uint64_t out_cap = dout ? c->mg.out_cap : 0;
    if (ntopics) {
        if (!d_store || !d_ret) return set_err(HVWS_EINVAL, "%s: null store", who);
        if ((uintptr_t)d_store & 15u) return set_err(HVWS_EINVAL, "%s: the store must be 16-byte aligned", who);
        if (ranges_overlap(d_store, store_len, d_ret, ret_len) || ranges_overlap(d_store, store_len, dout, out_cap) ||
            ranges_overlap(d_ret, ret_len, dout, out_cap) || ranges_overlap(d_store, store_len, src, src_cap) ||
            ranges_overlap(d_ret, ret_len, src, src_cap))
            return set_err(HVWS_EINVAL, "%s: the store, its entries and the message output overlap", who);
    }
    const uint64_t cap = c->rp.cap;   // < 2^32 - 1: hvws_route saw it
    const uint64_t np = std::min<uint64_t>(cap, ntopics) + 1;
    HIP_OR(p.scan.ensure(retain_scratch_bytes(cap)), HVWS_ENOMEM);
    HIP_OR(p.win.ensure((uint64_t)ntopics * 4 + 16), HVWS_ENOMEM);
    HIP_OR(p.plan.ensure(4 * np * 8), HVWS_ENOMEM);
    HIP_OR(p.rows.ensure((cap + 1) * sizeof(dtxmsg)), HVWS_ENOMEM);
    HIP_OR(p.topic.ensure((cap + 1) * 4), HVWS_ENOMEM);
    HIP_OR(p.reply.ensure((cap + 1) * 8), HVWS_ENOMEM);
    HIP_OR(p.first.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.count.ensure((uint64_t)nseg * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.meta.ensure(64), HVWS_ENOMEM);
    const retain_tables t{rows, c->rt.topic.as<uint32_t>(), c->rt.kind.as<uint8_t>(),
                          c->rt.scan.as<uint32_t>(), c->rt.ev.as<dsubev>(), c->rp.scan.as<uint64_t>() + cap, cap,
                          c->rp.first.as<uint64_t>(), c->rp.count.as<uint64_t>(), nseg, ntopics, src, src_cap, d_store,
                          slot, reinterpret_cast<dretained*>(d_ret)};
    uint64_t* plan = p.plan.as<uint64_t>();
    const retain_work w{p.win.as<uint32_t>(), p.scan.p, plan, plan + np, plan + 2 * np, plan + 3 * np,
                        p.rows.as<dtxmsg>(), p.topic.as<uint32_t>(), p.reply.as<uint64_t>(), p.first.as<uint64_t>(),
                        p.count.as<uint64_t>(), p.meta.as<uint64_t>()};
    // the timed device work (hvws_last_kernel_ms): the whole pass
    HIP_OR(timed_begin(c), HVWS_EHIP);
    HIP_OR(launch_retain(t, w, c->stream), HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    p.have = true;
    p.nseg = nseg;
    p.route = c->rt.seq;
    p.rep = c->rp.seq;
    p.msg = c->mg.seq;
    p.gen = c->scan_gen;
    return HVWS_OK;
}
}  // namespace

// Each topic's last publication of the turn into the caller's store, and the
// snapshot rows for the turn's subscribes (hvws_retain.hip): the pick, one
// scan, the finish, the copy.  No wait.
int hvws_retain(hvws_ctx* c, uint8_t* d_store, uint64_t slot, hvws_retained* d_ret, uint32_t flags) {
    int rc = check_ctx(c);
    if (rc) return rc;
    c->rn.have = false;   // the tables are being rewritten
    if (!route_valid(c)) return set_err(HVWS_EINVAL, "hvws_retain without a preceding hvws_route");
    if (flags) return set_err(HVWS_EINVAL, "hvws_retain: unknown flag bits");
    const uint8_t* dout = c->mg.dout;
    return retain_run(c, "hvws_retain", c->rt.rows.as<dtxmsg>(), dout, dout ? c->mg.out_cap : 0, d_store, slot, d_ret);
}

namespace {
// The last hvws_retain's snapshot tables stand: no route, reply call, message call or scan since.
bool retain_valid(const hvws_ctx* c) {
    return route_valid(c) && c->rn.have && c->rn.route == c->rt.seq && c->rn.rep == c->rp.seq && c->rn.msg == c->mg.seq &&
           c->rn.gen == c->scan_gen;
}
int retain_ctx(hvws_ctx* c) {
    if (int rc = check_ctx(c)) return rc;
    return retain_valid(c) ? HVWS_OK : set_err(HVWS_EINVAL, "no hvws_retain call yet");
}
}  // namespace

const hvws_tx_msg* hvws_retain_device(hvws_ctx* c) { return retain_valid(c) ? c->rn.rows.as<hvws_tx_msg>() : nullptr; }

const uint64_t* hvws_retain_count_device(hvws_ctx* c) { return retain_valid(c) ? c->rn.meta.as<uint64_t>() : nullptr; }

int64_t hvws_retain_count(hvws_ctx* c) {
    if (retain_ctx(c)) return -1;
    return read_count(c, c->rn.meta.as<uint64_t>(), "hvws_retain_count");
}

int hvws_get_retain(hvws_ctx* c, hvws_tx_msg* rows, uint32_t* topic, uint64_t* reply, uint64_t first, uint64_t n) {
    const int64_t have = hvws_retain_count(c);
    if (have < 0) return HVWS_EINVAL;
    if (first > (uint64_t)have || n > (uint64_t)have - first) return set_err(HVWS_EINVAL, "snapshot range out of bounds");
    if (n == 0) return HVWS_OK;
    return read_rows(c, {{rows, c->rn.rows.as<dtxmsg>() + first, n * sizeof(dtxmsg)},
                         {topic, c->rn.topic.as<uint32_t>() + first, n * 4},
                         {reply, c->rn.reply.as<uint64_t>() + first, n * 8}});
}

int hvws_get_segment_retain(hvws_ctx* c, uint64_t* first, uint64_t* count) {
    if (int rc = retain_ctx(c)) return rc;
    const uint64_t nseg = c->rn.nseg;
    return read_rows(c, {{first, c->rn.first.p, nseg * 8}, {count, c->rn.count.p, nseg * 8}});
}

int hvws_get_retain_totals(hvws_ctx* c, uint64_t out[5]) {
    if (int rc = retain_ctx(c)) return rc;
    if (!out) return set_err(HVWS_EINVAL, "hvws_get_retain_totals: null out");
    return read_rows(c, {{out, c->rn.meta.as<uint64_t>() + 1, 40}});
}

uint64_t hvws_retain_tile(void) { return RETAIN_TILE; }

static_assert(HVWS_ENV_HDR_MAX == 23 && HVWS_SEQ_HDR_MAX == 45 && ENV_TILE <= 0xFFFFFFFFull, "envelope constants");

namespace {
// out_cap + (hdr_max + 15) * reply capacity + 16 (include/hvws.h); 0 where 64 bits do not hold it
uint64_t envelope_bound(const hvws_ctx* c, uint32_t hdr_max = HVWS_ENV_HDR_MAX) {
    const uint64_t out_cap = c->mg.dout ? c->mg.out_cap : 0, cap = c->rp.cap;   // cap < 2^32 - 1: hvws_route saw it
    const uint64_t per = (hdr_max + 15u) * cap + 16u;
    return out_cap > ~0ull - per ? 0 : out_cap + per;
}
}  // namespace

uint64_t hvws_envelope_bound(hvws_ctx* c) { return route_valid(c) ? envelope_bound(c) : 0; }

uint32_t hvws_envelope_tile(void) { return (uint32_t)ENV_TILE; }

namespace {
// What hvws_envelope and hvws_envelope_sequenced share once the route (and the
// numbering) is known to stand: seq (null: hvws_envelope) is the number per
// reply, hdr_max the longest line of the form.
int envelope_run(hvws_ctx* c, const char* who, uint8_t* d_env, uint64_t env_cap, uint32_t flags, const uint64_t* seq,
                 uint32_t hdr_max) {
    pass_envelope& p = c->en;
    if (flags & ~(uint32_t)HVWS_ENV_SENDER) return set_err(HVWS_EINVAL, "%s: unknown flag bits", who);
    if (!d_env || ((uintptr_t)d_env & 15u)) return set_err(HVWS_EINVAL, "%s: d_env must be 16-byte aligned, not null", who);
    const uint64_t bound = envelope_bound(c, hdr_max);
    if (bound == 0 || env_cap < bound)
        return set_err(HVWS_EINVAL, "%s: env_cap = %llu, %s_bound %llu", who, (unsigned long long)env_cap, who,
                       (unsigned long long)bound);
    const uint8_t* dout = c->mg.dout;
    const uint64_t out_cap = dout ? c->mg.out_cap : 0;
    if (ranges_overlap(d_env, env_cap, dout, out_cap))
        return set_err(HVWS_EINVAL, "%s: d_env and the message output overlap", who);
    const uint64_t cap = c->rp.cap, np = cap + 1;
    HIP_OR(p.scan.ensure(env_scratch_bytes(cap)), HVWS_ENOMEM);
    HIP_OR(p.rows.ensure((cap + 1) * sizeof(dtxmsg)), HVWS_ENOMEM);
    HIP_OR(p.rrows.ensure((cap + 1) * sizeof(dtxmsg)), HVWS_ENOMEM);
    HIP_OR(p.plan.ensure(4 * np * 8), HVWS_ENOMEM);
    HIP_OR(p.meta.ensure(64), HVWS_ENOMEM);
    const env_tables t{c->rt.rows.as<dtxmsg>(), c->rt.topic.as<uint32_t>(), c->rt.kind.as<uint8_t>(),
                       c->rp.piece.as<uint64_t>(), c->rp.scan.as<uint64_t>() + cap, cap, c->mg.msgs.as<dmsg>(),
                       c->mg.meta.as<uint64_t>(), c->mg.cap, c->rt.nseg, c->rt.in.as<uint32_t>(), dout, out_cap, d_env,
                       env_cap, (flags & HVWS_ENV_SENDER) != 0, seq};
    uint64_t* plan = p.plan.as<uint64_t>();
    const env_work w{p.scan.p, p.rows.as<dtxmsg>(), p.rrows.as<dtxmsg>(), plan, plan + np, plan + 2 * np, plan + 3 * np,
                     p.meta.as<uint64_t>()};
    // the timed device work (hvws_last_kernel_ms): the whole pass
    HIP_OR(timed_begin(c), HVWS_EHIP);
    HIP_OR(launch_envelope(t, w, c->stream), HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    p.have = true;
    p.env = d_env;
    p.env_cap = env_cap;
    p.flags = flags;
    p.route = c->rt.seq;
    p.rep = c->rp.seq;
    p.msg = c->mg.seq;
    p.gen = c->scan_gen;
    return HVWS_OK;
}
}  // namespace

// Every reply's outgoing bytes into the caller's second buffer, publications
// behind their envelope line, and the rows that point there
// (hvws_envelope.hip): one scan, the finish, the copy.  No wait.
int hvws_envelope(hvws_ctx* c, uint8_t* d_env, uint64_t env_cap, uint32_t flags) {
    int rc = check_ctx(c);
    if (rc) return rc;
    c->en.have = false;   // the tables are being rewritten
    if (!route_valid(c)) return set_err(HVWS_EINVAL, "hvws_envelope without a preceding hvws_route");
    return envelope_run(c, "hvws_envelope", d_env, env_cap, flags, nullptr, HVWS_ENV_HDR_MAX);
}

namespace {
// The last hvws_envelope's tables stand: no route, reply call, message call or scan since.
bool envelope_valid(const hvws_ctx* c) {
    return route_valid(c) && c->en.have && c->en.route == c->rt.seq && c->en.rep == c->rp.seq && c->en.msg == c->mg.seq &&
           c->en.gen == c->scan_gen;
}
int envelope_ctx(hvws_ctx* c) {
    if (int rc = check_ctx(c)) return rc;
    return envelope_valid(c) ? HVWS_OK : set_err(HVWS_EINVAL, "no hvws_envelope call yet");
}
}  // namespace

const hvws_tx_msg* hvws_envelope_device(hvws_ctx* c) { return envelope_valid(c) ? c->en.rows.as<hvws_tx_msg>() : nullptr; }

int hvws_get_envelope(hvws_ctx* c, hvws_tx_msg* rows, uint64_t first, uint64_t n) {
    if (int rc = envelope_ctx(c)) return rc;
    const int64_t have = hvws_reply_count(c);
    if (have < 0) return HVWS_EINVAL;
    if (first > (uint64_t)have || n > (uint64_t)have - first) return set_err(HVWS_EINVAL, "reply range out of bounds");
    if (n == 0) return HVWS_OK;
    return read_rows(c, {{rows, c->en.rows.as<dtxmsg>() + first, n * sizeof(dtxmsg)}});
}

int hvws_get_envelope_totals(hvws_ctx* c, uint64_t out[4]) {
    if (int rc = envelope_ctx(c)) return rc;
    if (!out) return set_err(HVWS_EINVAL, "hvws_get_envelope_totals: null out");
    return read_rows(c, {{out, c->en.meta.as<uint64_t>(), 32}});
}

// hvws_fanout_routed delivering the rows of the last hvws_envelope.
int hvws_fanout_enveloped(hvws_ctx* c, const uint64_t* d_topic_first, const uint32_t* d_member, uint64_t nmember,
                          uint32_t flags, uint64_t max_deliveries, uint64_t* out_deliveries) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (out_deliveries) *out_deliveries = 0;
    c->fan.have = false;   // the tables are being rewritten
    c->bg.have = false;    // ... which a budget pass ran over
    if (!envelope_valid(c)) return set_err(HVWS_EINVAL, "hvws_fanout_enveloped without a preceding hvws_envelope");
    if (flags & ~(uint32_t)HVWS_FAN_SELF) return set_err(HVWS_EINVAL, "hvws_fanout_enveloped: unknown flag bits");
    if (c->rt.ntopics && (!d_topic_first || (!d_member && nmember)))
        return set_err(HVWS_EINVAL, "hvws_fanout_enveloped: null subscription table");
    const uint64_t cap = c->rp.cap;   // < 2^32 - 1: hvws_route saw it
    const fan_tables t{c->en.rows.as<dtxmsg>(), c->rp.piece.as<uint64_t>(), c->rp.scan.as<uint64_t>() + cap, cap,
                       c->mg.msgs.as<dmsg>(), c->mg.meta.as<uint64_t>(), c->mg.cap, c->rt.nseg, c->rt.in.as<uint32_t>(),
                       nullptr, d_topic_first, d_member, c->rt.ntopics, nmember, c->rt.ndest,
                       (flags & HVWS_FAN_SELF) != 0, c->rt.topic.as<uint32_t>()};
    if ((rc = fan_run(c, "hvws_fanout_enveloped", t, cap, max_deliveries, out_deliveries)) != HVWS_OK) return rc;
    c->fan.maxlen = c->en.env_cap;   // the rows point into d_env
    return HVWS_OK;
}

// hvws_retain keeping the enveloped bytes: the winners' rows are the envelope
// pass's (length 0 where the body is empty), their bytes are in d_env.
int hvws_retain_enveloped(hvws_ctx* c, uint8_t* d_store, uint64_t slot, hvws_retained* d_ret, uint32_t flags) {
    int rc = check_ctx(c);
    if (rc) return rc;
    c->rn.have = false;   // the tables are being rewritten
    if (!envelope_valid(c)) return set_err(HVWS_EINVAL, "hvws_retain_enveloped without a preceding hvws_envelope");
    if (flags) return set_err(HVWS_EINVAL, "hvws_retain_enveloped: unknown flag bits");
    return retain_run(c, "hvws_retain_enveloped", c->en.rrows.as<dtxmsg>(), c->en.env, c->en.env_cap, d_store, slot, d_ret);
}

// Every publication's number in its topic, and the caller's counters moved on
// (hvws_seq.hip): the pairs, the sort, one scan, the numbers, the counters.  No
// wait.
int hvws_sequence(hvws_ctx* c, uint64_t* d_seq, uint32_t flags) {
    int rc = check_ctx(c);
    if (rc) return rc;
    pass_sequence& p = c->sq;
    if (!route_valid(c)) return set_err(HVWS_EINVAL, "hvws_sequence without a preceding hvws_route");
    // a second numbering of one turn would skip numbers; the first one's table stands
    if (p.numbered == c->rt.seq) return set_err(HVWS_EINVAL, "hvws_sequence: this hvws_route's turn is numbered already");
    p.have = false;   // the table is being rewritten
    if (flags) return set_err(HVWS_EINVAL, "hvws_sequence: unknown flag bits");
    const uint32_t ntopics = c->rt.ntopics;
    const uint8_t* dout = c->mg.dout;
    const uint64_t out_cap = dout ? c->mg.out_cap : 0;
    if (ntopics) {
        if (!d_seq || ((uintptr_t)d_seq & 7u)) return set_err(HVWS_EINVAL, "hvws_sequence: d_seq must be 8-byte aligned, not null");
        if (ranges_overlap(d_seq, (uint64_t)ntopics * 8, dout, out_cap))
            return set_err(HVWS_EINVAL, "hvws_sequence: the counters and the message output overlap");
    }
    const uint64_t cap = c->rp.cap;   // < 2^32 - 1: hvws_route saw it
    HIP_OR(p.scan.ensure(seq_scratch_bytes(cap)), HVWS_ENOMEM);
    HIP_OR(p.ping.ensure(cap * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.pong.ensure(cap * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.hist.ensure(fan_hist_words(cap) * 8), HVWS_ENOMEM);
    HIP_OR(p.seq.ensure((cap + 1) * 8), HVWS_ENOMEM);
    HIP_OR(p.meta.ensure(64), HVWS_ENOMEM);
    const seq_tables t{c->rt.topic.as<uint32_t>(), c->rt.kind.as<uint8_t>(), c->rp.scan.as<uint64_t>() + cap, cap, ntopics,
                       d_seq};
    uint32_t* key[2] = {p.ping.as<uint32_t>(), p.pong.as<uint32_t>()};
    const seq_work w{{key[0], key[1]}, {key[0] + cap, key[1] + cap}, p.hist.as<uint64_t>(), p.scan.p, p.seq.as<uint64_t>(),
                     p.meta.as<uint64_t>()};
    // the timed device work (hvws_last_kernel_ms): the whole pass
    HIP_OR(timed_begin(c), HVWS_EHIP);
    HIP_OR(launch_sequence(t, w, c->stream), HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    p.have = true;
    p.numbered = c->rt.seq;
    p.route = c->rt.seq;
    p.rep = c->rp.seq;
    p.msg = c->mg.seq;
    p.gen = c->scan_gen;
    return HVWS_OK;
}

namespace {
// The last hvws_sequence's table stands: no route, reply call, message call or scan since.
bool sequence_valid(const hvws_ctx* c) {
    return route_valid(c) && c->sq.have && c->sq.route == c->rt.seq && c->sq.rep == c->rp.seq && c->sq.msg == c->mg.seq &&
           c->sq.gen == c->scan_gen;
}
int sequence_ctx(hvws_ctx* c) {
    if (int rc = check_ctx(c)) return rc;
    return sequence_valid(c) ? HVWS_OK : set_err(HVWS_EINVAL, "no hvws_sequence call yet");
}
}  // namespace

const uint64_t* hvws_sequence_device(hvws_ctx* c) { return sequence_valid(c) ? c->sq.seq.as<uint64_t>() : nullptr; }

int hvws_get_sequence(hvws_ctx* c, uint64_t* seq, uint64_t first, uint64_t n) {
    if (int rc = sequence_ctx(c)) return rc;
    const int64_t have = hvws_reply_count(c);
    if (have < 0) return HVWS_EINVAL;
    if (first > (uint64_t)have || n > (uint64_t)have - first) return set_err(HVWS_EINVAL, "reply range out of bounds");
    if (n == 0) return HVWS_OK;
    return read_rows(c, {{seq, c->sq.seq.as<uint64_t>() + first, n * 8}});
}

int hvws_get_sequence_totals(hvws_ctx* c, uint64_t out[2]) {
    if (int rc = sequence_ctx(c)) return rc;
    if (!out) return set_err(HVWS_EINVAL, "hvws_get_sequence_totals: null out");
    return read_rows(c, {{out, c->sq.meta.as<uint64_t>(), 16}});
}

uint64_t hvws_envelope_sequenced_bound(hvws_ctx* c) { return route_valid(c) ? envelope_bound(c, HVWS_SEQ_HDR_MAX) : 0; }

// hvws_envelope whose publication lines end in the number the last
// hvws_sequence gave (hvws_envelope.hip, the sequenced form).  Fills the
// tables of hvws_envelope.  No wait.
int hvws_envelope_sequenced(hvws_ctx* c, uint8_t* d_env, uint64_t env_cap, uint32_t flags) {
    int rc = check_ctx(c);
    if (rc) return rc;
    c->en.have = false;   // the tables are being rewritten
    if (!route_valid(c)) return set_err(HVWS_EINVAL, "hvws_envelope_sequenced without a preceding hvws_route");
    if (!sequence_valid(c)) return set_err(HVWS_EINVAL, "hvws_envelope_sequenced without a preceding hvws_sequence");
    return envelope_run(c, "hvws_envelope_sequenced", d_env, env_cap, flags, c->sq.seq.as<uint64_t>(), HVWS_SEQ_HDR_MAX);
}

static_assert(BF_OVER == HVWS_BF_OVER, "budget flag bits");

// The last hvws_fanout's deliveries cut at every destination's byte budget
// (hvws_budget.hip): the size scan, the cut, two scans over the destinations,
// the placement.  No wait: the fan-out's delivery count is on the host already.
int hvws_budget(hvws_ctx* c, const uint64_t* d_budget, uint64_t budget_all, uint64_t fragment, int masked) {
    int rc = check_ctx(c);
    if (rc) return rc;
    c->bg.have = false;   // the tables are being rewritten
    if (!fan_valid(c)) return set_err(HVWS_EINVAL, "hvws_budget without a preceding hvws_fanout");
    if (c->rp.gen != c->scan_gen) return set_err(HVWS_EINVAL, "hvws_budget: a scan has run since hvws_replies");
    if (masked != 0 && masked != 1) return set_err(HVWS_EINVAL, "hvws_budget: masked = %d (0 or 1)", masked);
    const uint64_t n = c->fan.n;
    const uint32_t ndest = c->fan.ndest;
    const uint64_t F = fragment ? fragment : 0xFFFFu;   // WebSocketChannel.cpp:6
    // no row names more than the bytes of the buffer it points into (the message
    // call's out_cap; env_cap behind hvws_fanout_enveloped): n messages of that
    // length bound every sum the kernels form
    const uint64_t maxlen = c->fan.maxlen, wmax = budget_wire(maxlen, F, masked);
    if (n && (wmax == ~0ull || wmax > ~0ull / n))
        return set_err(HVWS_EINVAL, "hvws_budget: %llu deliveries of up to %llu bytes do not fit 64 bits",
                       (unsigned long long)n, (unsigned long long)wmax);
    pass_budget& p = c->bg;
    HIP_OR(p.scan.ensure(budget_scratch_words(n, ndest) * 8), HVWS_ENOMEM);
    HIP_OR(p.cnt.ensure((uint64_t)ndest * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.kept.ensure((uint64_t)ndest * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.flags.ensure((uint64_t)ndest + 16), HVWS_ENOMEM);
    HIP_OR(p.first.ensure(((uint64_t)ndest + 1) * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.off.ensure(((uint64_t)ndest + 1) * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.msgs.ensure((n + 1) * sizeof(dtxmsg)), HVWS_ENOMEM);
    HIP_OR(p.reply.ensure((n + 1) * 8), HVWS_ENOMEM);
    HIP_OR(p.meta.ensure(64), HVWS_ENOMEM);
    const uint32_t* key = (c->fan.key_in ? c->fan.pong : c->fan.ping).as<uint32_t>();
    const budget_tables t{c->fan.msgs.as<dtxmsg>(), c->fan.reply.as<uint64_t>(), key, n, c->fan.first.as<uint64_t>(),
                          c->fan.count.as<uint64_t>(), ndest, d_budget, budget_all, F, maxlen, masked != 0};
    const budget_work w{p.scan.as<uint64_t>(), p.cnt.as<uint64_t>(), p.kept.as<uint64_t>(), p.flags.as<uint8_t>(),
                        p.first.as<uint64_t>(), p.off.as<uint64_t>(), p.msgs.as<dtxmsg>(), p.reply.as<uint64_t>(),
                        p.meta.as<uint64_t>()};
    // the timed device work (hvws_last_kernel_ms): the whole pass
    HIP_OR(timed_begin(c), HVWS_EHIP);
    HIP_OR(launch_budget(t, w, c->stream), HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    p.have = true;
    p.ndest = ndest;
    p.n = n;
    p.rep = c->fan.rep;
    p.msg = c->fan.msg;
    p.gen = c->scan_gen;
    return HVWS_OK;
}

namespace {
// The last hvws_budget's tables stand: its fan-out's do, and no scan since.
bool budget_valid(const hvws_ctx* c) {
    return fan_valid(c) && c->bg.have && c->bg.rep == c->fan.rep && c->bg.msg == c->fan.msg && c->bg.gen == c->scan_gen;
}
}  // namespace

const hvws_tx_msg* hvws_budget_device(hvws_ctx* c) { return budget_valid(c) ? c->bg.msgs.as<hvws_tx_msg>() : nullptr; }

const uint64_t* hvws_budget_count_device(hvws_ctx* c) { return budget_valid(c) ? c->bg.meta.as<uint64_t>() : nullptr; }

int64_t hvws_budget_count(hvws_ctx* c) {
    if (check_ctx(c)) return -1;
    if (!budget_valid(c)) {
        set_err(HVWS_EINVAL, "no hvws_budget call yet");
        return -1;
    }
    return read_count(c, c->bg.meta.as<uint64_t>(), "hvws_budget_count");
}

int hvws_get_budget(hvws_ctx* c, hvws_tx_msg* out, uint64_t* reply, uint64_t first, uint64_t n) {
    const int64_t have = hvws_budget_count(c);
    if (have < 0) return HVWS_EINVAL;
    if (first > (uint64_t)have || n > (uint64_t)have - first)
        return set_err(HVWS_EINVAL, "kept delivery range out of bounds");
    if (n == 0) return HVWS_OK;
    return read_rows(c, {{out, c->bg.msgs.as<dtxmsg>() + first, n * sizeof(dtxmsg)},
                         {reply, c->bg.reply.as<uint64_t>() + first, n * 8}});
}

int hvws_get_dest_budget(hvws_ctx* c, uint64_t* first, uint64_t* count, uint64_t* byte_off, uint8_t* flags) {
    if (int rc = check_ctx(c)) return rc;
    if (!budget_valid(c)) return set_err(HVWS_EINVAL, "no hvws_budget call yet");
    const uint64_t nd = c->bg.ndest;
    return read_rows(c, {{first, c->bg.first.p, nd * 8},
                         {count, c->bg.cnt.p, nd * 8},
                         {byte_off, c->bg.off.p, (nd + 1) * 8},
                         {flags, c->bg.flags.p, nd}});
}

int hvws_get_budget_totals(hvws_ctx* c, uint64_t out[4]) {
    if (int rc = check_ctx(c)) return rc;
    if (!budget_valid(c)) return set_err(HVWS_EINVAL, "no hvws_budget call yet");
    if (!out) return set_err(HVWS_EINVAL, "hvws_get_budget_totals: null out");
    return read_rows(c, {{out, c->bg.meta.p, 32}});
}

static_assert(HVWS_SUB_JOIN == 1u && HVWS_SUB_LEAVE == 2u && HVWS_SUB_DROP == 3u && HVWS_SUBS_UNIQUE == 1u &&
                  sizeof(hvws_sub_event) == 12 && sizeof(dsubev) == sizeof(hvws_sub_event) &&
                  RF_CLOSED == HVWS_RF_CLOSED,
              "subscription update constants");

static_assert(HVWS_SUBS_OVER == 2u, "subscription update flag bits");

namespace {
bool ranges_meet(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}

// What hvws_subs_update and hvws_subs_update_routed refuse about the caller's
// arrays before anything is launched.
int subs_check_tables(const char* who, const uint64_t* d_topic_first, const uint32_t* d_member, uint32_t ntopics,
                      uint64_t nmember, const hvws_sub_event* events, uint64_t nev, uint64_t* d_topic_first_out,
                      uint32_t* d_member_out, uint64_t member_cap) {
    if (!d_topic_first || !d_topic_first_out || (!d_member && nmember) || (!d_member_out && member_cap) ||
        (!events && nev))
        return set_err(HVWS_EINVAL, "%s: null table", who);
    if (((uintptr_t)d_topic_first_out & 15u) || ((uintptr_t)d_member_out & 15u))
        return set_err(HVWS_EINVAL, "%s: the output arrays must be 16-byte aligned", who);
    const uint64_t fb = ((uint64_t)ntopics + 1) * 8, mb = std::min<uint64_t>(member_cap, 1ull << 32) * 4;
    if (ranges_meet(d_topic_first_out, fb, d_topic_first, fb) || ranges_meet(d_topic_first_out, fb, d_member, nmember * 4) ||
        ranges_meet(d_member_out, mb, d_topic_first, fb) || ranges_meet(d_member_out, mb, d_member, nmember * 4) ||
        ranges_meet(d_member_out, mb, d_topic_first_out, fb))
        return set_err(HVWS_EINVAL, "%s: an output array overlaps another array of the call", who);
    return HVWS_OK;
}

// ... and about the host's events.
int subs_check_events(const char* who, const hvws_sub_event* events, uint64_t nev, uint32_t ntopics, uint32_t ndest) {
    for (uint64_t e = 0; e < nev; ++e) {
        const hvws_sub_event& v = events[e];
        if (v.op < HVWS_SUB_JOIN || v.op > HVWS_SUB_DROP)
            return set_err(HVWS_EINVAL, "%s: events[%llu].op = %u", who, (unsigned long long)e, v.op);
        if (v.op != HVWS_SUB_DROP && v.topic >= ntopics)
            return set_err(HVWS_EINVAL, "%s: events[%llu].topic = %u of %u topics", who, (unsigned long long)e, v.topic,
                           ntopics);
        if (v.dest >= ndest)
            return set_err(HVWS_EINVAL, "%s: events[%llu].dest = %u of %u destinations", who, (unsigned long long)e,
                           v.dest, ndest);
    }
    return HVWS_OK;
}

// What the two calls share once their events stand in device memory (t.ev,
// t.nev of them): the work areas, the counting kernels, the one wait, the
// placement.
int subs_run(hvws_ctx* c, const char* who, const subs_tables& t, uint64_t* d_topic_first_out, uint32_t* d_member_out,
             uint64_t member_cap, uint64_t* out_nmember) {
    int rc;
    pass_subs& p = c->subs;
    const uint64_t nev = t.nev, nmember = t.nmember;
    HIP_OR(p.drop.ensure((uint64_t)t.ndest * 4 + 16), HVWS_ENOMEM);
    HIP_OR(p.ping.ensure(nev * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.pong.ensure(nev * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.hist.ensure(fan_hist_words(nev) * 8), HVWS_ENOMEM);
    HIP_OR(p.pk.ensure(nev * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.evfirst.ensure(((uint64_t)t.ntopics + 1) * 8 + 16), HVWS_ENOMEM);
    HIP_OR(p.bits.ensure(nev * 3 + 16), HVWS_ENOMEM);
    HIP_OR(p.surv.ensure(nmember + 16), HVWS_ENOMEM);
    HIP_OR(p.brow.ensure((nmember / 256 + 2) * 4 + 16), HVWS_ENOMEM);
    HIP_OR(p.erank.ensure(subs_event_rank_words(nev) * 8), HVWS_ENOMEM);
    HIP_OR(p.lrank.ensure(subs_rank_words(nmember) * 8), HVWS_ENOMEM);
    HIP_OR(p.meta.ensure(128), HVWS_ENOMEM);
    uint32_t* key0 = p.ping.as<uint32_t>();
    uint32_t* key1 = p.pong.as<uint32_t>();
    uint8_t* bits = p.bits.as<uint8_t>();
    const subs_work w{p.drop.as<uint32_t>(), {key0, key1}, {key0 + nev, key1 + nev}, p.hist.as<uint64_t>(),
                      p.pk.as<uint64_t>(), p.evfirst.as<uint64_t>(), bits, bits + nev, bits + 2 * nev, p.surv.as<uint8_t>(), p.brow.as<uint32_t>(),
                      p.erank.as<uint64_t>(), p.lrank.as<uint64_t>(), p.meta.as<uint64_t>()};
    HIP_OR(launch_subs_count(t, w, c->stream), HVWS_EHIP);
    // the one wait: new nmember, kept, added, removed, destinations dropped as closed, bad
    uint64_t h[6] = {0, 0, 0, 0, 0, 0};
    if ((rc = read_rows(c, {{h, w.meta, sizeof h}})) != HVWS_OK) return rc;
    if (h[5])
        return set_err(HVWS_EINVAL, "%s: the table is not dense (topic_first[0] != 0, a decreasing pair, "
                       "topic_first[ntopics] != nmember) or holds a member id outside the destinations", who);
    if (out_nmember) *out_nmember = h[0];
    if (h[0] > member_cap)
        return set_err(HVWS_EINVAL, "%s: %llu listings, member_cap %llu", who, (unsigned long long)h[0],
                       (unsigned long long)member_cap);
    // the timed device work (hvws_last_kernel_ms): the placement
    HIP_OR(timed_begin(c), HVWS_EHIP);
    HIP_OR(launch_subs_place(t, w, h[0], d_topic_first_out, d_member_out, c->stream), HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    p.have = true;
    memcpy(p.h, h, sizeof h);
    return HVWS_OK;
}
}  // namespace

// The next subscription table from the current one (hvws_subs.hip): drops,
// the pair sort, survive and effective bits and their scans, one wait for the
// counts, then the placement.
int hvws_subs_update(hvws_ctx* c, const uint64_t* d_topic_first, const uint32_t* d_member, uint32_t ntopics,
                     uint64_t nmember, uint32_t ndest, const hvws_sub_event* events, uint64_t nev,
                     const uint32_t* dest_of, uint32_t flags, uint64_t* d_topic_first_out, uint32_t* d_member_out,
                     uint64_t member_cap, uint64_t* out_nmember) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (out_nmember) *out_nmember = 0;
    c->subs.have = false;
    c->subs.merged = false;
    if (flags & ~(uint32_t)HVWS_SUBS_UNIQUE) return set_err(HVWS_EINVAL, "hvws_subs_update: unknown flag bits");
    if (ndest == 0 || ndest > 0x7FFFFFFFu)
        return set_err(HVWS_EINVAL, "hvws_subs_update: %u destinations (1 .. 2^31-1)", ndest);
    if (nmember > 0xFFFFFFFEull || nev > 0xFFFFFFFEull)
        return set_err(HVWS_EINVAL, "hvws_subs_update: %llu listings, %llu events (max 2^32-2 each)",
                       (unsigned long long)nmember, (unsigned long long)nev);
    if ((rc = subs_check_tables("hvws_subs_update", d_topic_first, d_member, ntopics, nmember, events, nev,
                                d_topic_first_out, d_member_out, member_cap)) != HVWS_OK)
        return rc;
    if ((rc = subs_check_events("hvws_subs_update", events, nev, ntopics, ndest)) != HVWS_OK) return rc;
    uint32_t nseg = 0;
    if (dest_of) {
        if (!c->rp.have) return set_err(HVWS_EINVAL, "hvws_subs_update: dest_of without a preceding hvws_replies");
        if (c->rp.gen != c->scan_gen)
            return set_err(HVWS_EINVAL, "hvws_subs_update: a scan has run since hvws_replies");
        nseg = c->rp.nseg;
        for (uint32_t s = 0; s < nseg; ++s)
            if (dest_of[s] >= ndest)
                return set_err(HVWS_EINVAL, "hvws_subs_update: dest_of[%u] = %u of %u destinations", s, dest_of[s], ndest);
    }
    pass_subs& p = c->subs;
    HIP_OR(p.in.ensure(nev * 12 + (uint64_t)nseg * 4 + 16), HVWS_ENOMEM);
    // the events, then dest_of behind them
    const bool drops = dest_of && nseg;
    if (nev)
        rc = p.up.send(p.in.p, c->stream, events, nev * 12, drops ? dest_of : nullptr, drops ? (uint64_t)nseg * 4 : 0);
    else
        rc = p.up.send(p.in.p, c->stream, drops ? dest_of : nullptr, (uint64_t)nseg * 4);
    if (rc != HVWS_OK) return rc;
    const subs_tables t{d_topic_first, d_member, ntopics, nmember, ndest, p.in.as<dsubev>(), nev,
                        drops ? reinterpret_cast<const uint32_t*>(p.in.as<uint8_t>() + nev * 12) : nullptr,
                        drops ? c->rp.flags.as<uint8_t>() : nullptr, drops ? nseg : 0u,
                        (flags & HVWS_SUBS_UNIQUE) != 0};
    return subs_run(c, "hvws_subs_update", t, d_topic_first_out, d_member_out, member_cap, out_nmember);
}

// hvws_subs_update over the turn's own events, merged on the device
// (hvws_subs.hip): the route's events, a DROP per closed or malformed
// connection, with HVWS_SUBS_OVER a DROP per destination the budget cut, then
// the host's events.  One wait for the merged count, then subs_run.
int hvws_subs_update_routed(hvws_ctx* c, const uint64_t* d_topic_first, const uint32_t* d_member, uint64_t nmember,
                            const hvws_sub_event* events, uint64_t nev, uint32_t flags, uint64_t* d_topic_first_out,
                            uint32_t* d_member_out, uint64_t member_cap, uint64_t* out_nmember) {
    const char* who = "hvws_subs_update_routed";
    int rc = check_ctx(c);
    if (rc) return rc;
    if (out_nmember) *out_nmember = 0;
    pass_subs& p = c->subs;
    p.have = false;
    p.merged = false;
    if (!route_valid(c)) return set_err(HVWS_EINVAL, "%s without a preceding hvws_route", who);
    if (flags & ~(uint32_t)(HVWS_SUBS_UNIQUE | HVWS_SUBS_OVER)) return set_err(HVWS_EINVAL, "%s: unknown flag bits", who);
    const bool over = (flags & HVWS_SUBS_OVER) != 0;
    const uint32_t ntopics = c->rt.ntopics, ndest = c->rt.ndest, nseg = c->rt.nseg;
    if (over && !budget_valid(c)) return set_err(HVWS_EINVAL, "%s: HVWS_SUBS_OVER without a preceding hvws_budget", who);
    if (over && c->bg.ndest != ndest)
        return set_err(HVWS_EINVAL, "%s: hvws_budget ran over %u destinations, hvws_route over %u", who, c->bg.ndest, ndest);
    if (nmember > 0xFFFFFFFEull || nev > 0xFFFFFFFEull)
        return set_err(HVWS_EINVAL, "%s: %llu listings, %llu events (max 2^32-2 each)", who, (unsigned long long)nmember,
                       (unsigned long long)nev);
    if ((rc = subs_check_tables(who, d_topic_first, d_member, ntopics, nmember, events, nev, d_topic_first_out,
                                d_member_out, member_cap)) != HVWS_OK)
        return rc;
    if ((rc = subs_check_events(who, events, nev, ntopics, ndest)) != HVWS_OK) return rc;
    const uint64_t cap = c->rp.cap;   // < 2^32 - 1: hvws_route saw it
    const uint32_t nover = over ? ndest : 0u;
    HIP_OR(p.in.ensure(nev * 12 + 16), HVWS_ENOMEM);
    HIP_OR(p.mev.ensure((cap + nseg + nover + nev + 1) * sizeof(dsubev)), HVWS_ENOMEM);
    HIP_OR(p.mscan.ensure(subs_merge_words(nseg, nover) * 8), HVWS_ENOMEM);
    HIP_OR(p.mcnt.ensure(64), HVWS_ENOMEM);
    if ((rc = p.up.send(p.in.p, c->stream, events, nev * 12)) != HVWS_OK) return rc;
    const subs_merge mt{c->rt.ev.as<dsubev>(), c->rt.meta.as<uint64_t>(), cap, c->rp.flags.as<uint8_t>(),
                        c->rt.flags.as<uint8_t>(), c->rt.in.as<uint32_t>(), nseg,
                        over ? c->bg.flags.as<uint8_t>() : nullptr, nover, p.in.as<dsubev>(), nev};
    HIP_OR(launch_subs_merge(mt, p.mscan.as<uint64_t>(), p.mev.as<dsubev>(), p.mcnt.as<uint64_t>(), c->stream), HVWS_EHIP);
    // the first wait: route events, connection drops, OVER drops, host events, their sum
    uint64_t m[5] = {0, 0, 0, 0, 0};
    if ((rc = read_rows(c, {{m, p.mcnt.p, sizeof m}})) != HVWS_OK) return rc;
    if (m[4] > 0xFFFFFFFEull)
        return set_err(HVWS_EINVAL, "%s: %llu merged events (max 2^32-2)", who, (unsigned long long)m[4]);
    p.merged = true;
    memcpy(p.m, m, sizeof m);
    const subs_tables t{d_topic_first, d_member, ntopics, nmember, ndest, p.mev.as<dsubev>(), m[4], nullptr, nullptr, 0u,
                        (flags & HVWS_SUBS_UNIQUE) != 0};
    return subs_run(c, who, t, d_topic_first_out, d_member_out, member_cap, out_nmember);
}

int hvws_get_subs_merged(hvws_ctx* c, uint64_t out[4]) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->subs.merged) return set_err(HVWS_EINVAL, "no hvws_subs_update_routed call yet");
    if (!out) return set_err(HVWS_EINVAL, "hvws_get_subs_merged: null out");
    for (int k = 0; k < 4; ++k) out[k] = c->subs.m[k];
    return HVWS_OK;
}

int hvws_get_subs_events(hvws_ctx* c, hvws_sub_event* out, uint64_t first, uint64_t n) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->subs.merged) return set_err(HVWS_EINVAL, "no hvws_subs_update_routed call yet");
    const uint64_t have = c->subs.m[4];
    if (first > have || n > have - first) return set_err(HVWS_EINVAL, "merged event range out of bounds");
    if (n == 0) return HVWS_OK;
    return read_rows(c, {{out, c->subs.mev.as<dsubev>() + first, n * sizeof(dsubev)}});
}

int64_t hvws_subs_count(hvws_ctx* c) {
    if (check_ctx(c)) return -1;
    if (!c->subs.have) {
        set_err(HVWS_EINVAL, "no hvws_subs_update call yet");
        return -1;
    }
    return (int64_t)c->subs.h[0];
}

int hvws_get_subs_counts(hvws_ctx* c, uint64_t out[4]) {
    if (int rc = check_ctx(c)) return rc;
    if (!c->subs.have) return set_err(HVWS_EINVAL, "no hvws_subs_update call yet");
    if (!out) return set_err(HVWS_EINVAL, "hvws_get_subs_counts: null out");
    for (int k = 0; k < 4; ++k) out[k] = c->subs.h[1 + k];
    return HVWS_OK;
}

int hvws_encode_keys(hvws_ctx* c, const char* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
                     uint64_t n, char* d_accept) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (n == 0) return HVWS_OK;
    if (!d_keys || !d_key_off || !d_key_len || !d_accept) return set_err(HVWS_EINVAL, "encode_keys: null table");
    if (((uintptr_t)d_accept & 15u) != 0) return set_err(HVWS_EINVAL, "encode_keys: accept buffer must be 16-byte aligned");
    HIP_OR(timed_begin(c), HVWS_EHIP);
    HIP_OR(launch_encode_keys((const uint8_t*)d_keys, d_key_off, d_key_len, n, (uint8_t*)d_accept, c->stream),
           HVWS_EHIP);
    HIP_OR(timed_end(c), HVWS_EHIP);
    return HVWS_OK;
}

int hvws_last_kernel_ms(hvws_ctx* c, float* ms) {
    int rc = check_ctx(c);
    if (rc) return rc;
    if (!c->ev_build) return set_err(HVWS_EINVAL, "no build_frames / encode_keys / utf8 call yet");
    HIP_OR(hipEventSynchronize(c->ev[5]), HVWS_EHIP);
    HIP_OR(hipEventElapsedTime(ms, c->ev[4], c->ev[5]), HVWS_EHIP);
    return HVWS_OK;
}

const char* hvws_build_kernel_name(void) { return build_kernel_name(tx_variant(0, 0)); }

const char* hvws_last_build_kernel(hvws_ctx* c) {
    if (!c) return "";
    return build_kernel_name(c->tx.variant);
}

int hvws_last_build_uniform(hvws_ctx* c) { return c && c->tx.uniform ? 1 : 0; }

uint32_t hvws_set_validation(hvws_ctx* c, uint32_t classes) {
    if (!c) c = hvws::thread_ctx();
    const uint32_t old = c->vmask;
    c->vmask = classes & V_ALL;
    return old;
}

int hvws_set_door(hvws_ctx* c, int on) {
    if (!c) c = hvws::thread_ctx();
    std::lock_guard<std::mutex> cl(c->door_m);
    const int old = door_on(c) ? 1 : 0;
    c->door_mode = on < 0 ? -1 : (on ? 1 : 0);
    if (!door_on(c) && c->door_live) {   // off (explicitly, or -1 resolving to off): park now
        int dev = -1;
        (void)hipGetDevice(&dev);
        hipSetDevice(c->device);
        door_park(c);
        if (dev >= 0) hipSetDevice(dev);
    }
    return old;
}

int hvws_door_info(hvws_ctx* c, uint64_t out[2]) {
    if (!c) c = hvws::thread_ctx();
    if (!out) return set_err(HVWS_EINVAL, "null output");
    out[0] = c->d_door_req ? 1 : 0;
    out[1] = c->door_q ? 1 : 0;
    return HVWS_OK;
}

int hvws_door_stamps(hvws_ctx* c, uint64_t out[12]) {
    if (!c) c = hvws::thread_ctx();
    if (!out) return set_err(HVWS_EINVAL, "null output");
    memset(out, 0, 12 * sizeof(uint64_t));
    if (c->h_door.p) memcpy(out, c->h_door.as<ddoor>()->stamp, 12 * sizeof(uint64_t));
    return HVWS_OK;
}

uint64_t hvws_set_door_idle_us(uint64_t us) {
    const uint64_t old = door_idle_us();
    g_door_idle_us.store(us ? us : 5000, std::memory_order_relaxed);
    return old;
}

int hvws_door_health(uint64_t out[2]) {
    if (!out) return set_err(HVWS_EINVAL, "null output");
    out[0] = g_door_wedged.load();
    out[1] = g_door_failed.load();
    return HVWS_OK;
}

int hvws_door_stats(hvws_ctx* c, uint64_t out[4]) {
    if (!c) c = hvws::thread_ctx();
    if (!out) return set_err(HVWS_EINVAL, "null output");
    out[0] = c->door_launches;
    out[1] = c->door_calls;
    out[2] = c->h_door.p ? __atomic_load_n(&c->h_door.as<ddoor>()->served, __ATOMIC_ACQUIRE) : 0;
    out[3] = c->door_live ? 1 : 0;
    return HVWS_OK;
}

uint64_t hvws_set_small_batch_limit(hvws_ctx* c, uint64_t bytes) {
    if (!c) c = hvws::thread_ctx();   // the calling thread's reference-API context
    const uint64_t old = c->small_limit ? c->small_limit : kSmallBatch;
    c->small_limit = bytes;
    return old;
}

int hvws_set_small_zero_copy(hvws_ctx* c, int on) {
    if (!c) c = hvws::thread_ctx();
    const int old = c->small_zc;
    c->small_zc = on ? 1 : 0;
    return old;
}

const char* hvws_unmask_kernel_name(void) { return unmask_name(unmask_variant()); }

const char* hvws_unmask_kernel_name_for(uint64_t rx_len) { return unmask_name(unmask_variant_for(rx_len)); }

const char* hvws_run_kernel_name(void) { return run_kernel_name(); }

uint64_t hvws_set_spec_min(uint64_t frames) { return set_spec_min(frames); }

uint64_t hvws_set_sieve_min(uint64_t bytes) { return set_sieve_min(bytes); }

int hvws_set_table_checks(int on) {
    const int prev = table_checks() ? 1 : 0;
    __atomic_store_n(&g_table_checks, on ? 1 : 0, __ATOMIC_RELAXED);
    return prev;
}

int hvws_last_sieve(hvws_ctx* c, uint64_t out[4]) {
    if (!c) c = thread_ctx();
    if (!c || !out) return set_err(HVWS_EINVAL, "hvws_last_sieve: NULL argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!c->sv_ran) return HVWS_OK;
    HIP_OR(hipSetDevice(c->device), HVWS_EHIP);
    HIP_OR(hipStreamSynchronize(c->cs), HVWS_EHIP);
    const dsieve* d = c->h_sv.as<dsieve>();
    const uint64_t* n = reinterpret_cast<const uint64_t*>(c->h_sv.as<uint8_t>() + sizeof(dsieve));
    out[0] = d->active ? (n[3] <= c->sv_cap && n[0] <= c->sv_capc ? 1 : 2) : 0;
    out[1] = d->active ? n[0] : 0;
    out[2] = d->use ? d->npath : 0;
    out[3] = d->use ? d->pend : 0;
    return HVWS_OK;
}

void hvws_set_sieve_windows(uint64_t hops, uint64_t window_bytes, uint64_t prev[2]) {
    set_sieve_windows(hops, window_bytes, prev);
}

int hvws_last_sieve_windows(hvws_ctx* c, uint64_t out[2]) {
    if (!c) c = thread_ctx();
    if (!c || !out) return set_err(HVWS_EINVAL, "hvws_last_sieve_windows: NULL argument");
    out[0] = c->sv_ran ? c->sv_rt : 0;
    out[1] = c->sv_ran ? c->sv_wt : 0;
    return HVWS_OK;
}

int hvws_last_scan_path(hvws_ctx* c) { return c ? c->scan_path : -1; }

uint64_t hvws_set_fast_bound(hvws_ctx* c, uint64_t records) {
    if (!c) return 0;
    const uint64_t old = c->fast_bound ? c->fast_bound : kFastFrameBound;
    c->fast_bound = records;
    return old;
}

int hvws_set_walk_verify(hvws_ctx* c, int mode) {
    if (!c) c = thread_ctx();
    if (!c) return HVWS_ENODEV;
    const int old = c->verify_mode;
    c->verify_mode = mode < 0 ? -1 : (mode ? 1 : 0);
    return old;
}

int64_t hvws_last_run_repairs(hvws_ctx* c) {
    if (check_ctx(c) != HVWS_OK || c->scan_path != HVWS_PATH_RUN) return -1;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    const dspec_status* st = c->h_status.as<dspec_status>();
    return __atomic_load_n(&st->run_seq, __ATOMIC_ACQUIRE) == c->run_seq ? (int64_t)st->run_failed : -1;
}

int hvws_set_run(hvws_ctx* c, int mode) {
    if (!c) c = thread_ctx();
    if (!c) return HVWS_ENODEV;
    const int old = c->run_mode;
    c->run_mode = mode < 0 ? -1 : (mode ? 1 : 0);
    return old;
}

int hvws_set_speculation(hvws_ctx* c, int mode) {
    if (!c) c = thread_ctx();
    if (!c) return HVWS_ENODEV;
    const int old = c->spec_mode;
    c->spec_mode = mode < 0 ? -1 : (mode > 2 ? 2 : mode);
    return old;
}

int hvws_set_unmask_variant(int v) {
    if (set_unmask_variant(v) < -1) return set_err(HVWS_EINVAL, "unmask variant %d out of range [-1,%d)", v,
                                                   unmask_variant_count());
    return HVWS_OK;
}

void hvws_thread_release(void) {
    if (t_ctx) hvws_ctx_destroy(t_ctx);
    t_ctx = nullptr;
}

int hvws_set_thread_device(int device) {
    if (t_ctx && t_ctx->device != device) {
        hvws_ctx_destroy(t_ctx);
        t_ctx = nullptr;
    }
    t_device = device;
    return HVWS_OK;
}

}  // extern "C"

// ----------------------------------------------- internal helpers for the drop-in
namespace hvws {

[[noreturn]] void fatal(const char* what) {
    fprintf(stderr, "libhvws: %s: %s -- the MI355X WebSocket path has no CPU fallback\n", what, g_err);
    fflush(stderr);
    abort();
}

// Parks the thread context's resident worker when the thread exits (the
// context itself lives on until hvws_thread_release, as before).
// The main thread's guard runs inside exit(): it only asks the worker to
// exit through the mailbox (no HIP call, like door_atexit).
struct thread_door_guard {
    ~thread_door_guard() {
        if (!t_ctx || !t_ctx->door_live) return;
        std::lock_guard<std::mutex> cl(t_ctx->door_m);
        if ((pid_t)syscall(SYS_gettid) == getpid()) {
            door_quit_nohip(t_ctx);
        } else {
            hipSetDevice(t_ctx->device);
            door_park(t_ctx);
        }
    }
};
thread_local thread_door_guard t_door_guard;

hvws_ctx* thread_ctx() {
    if (t_ctx) return t_ctx;
    (void)&t_door_guard;
    int dev = t_device;
    if (dev < 0) {
        const char* e = getenv("HVWS_DEVICE");
        dev = e ? atoi(e) : 0;
    }
    t_ctx = hvws_ctx_create(dev);
    if (!t_ctx) fatal("cannot open a HIP device context");
    return t_ctx;
}

// A feeder's worker context takes the per-context knobs of the thread that
// made the feeder (small-batch path, zero-copy, validation classes).
void ctx_copy_settings(hvws_ctx* dst, const hvws_ctx* src) {
    dst->small_limit = src->small_limit;
    dst->small_zc = src->small_zc;
    dst->zc_batch = src->zc_batch;
    dst->vmask = src->vmask;
}

// The host record cache of the last small-path call, moved out (no copy) with
// its per-segment first/count; the context then holds no scan (the batched
// drop-in is the only reader of its thread context's records).
bool take_frames(hvws_ctx* c, std::vector<hvws_frame>& frames, std::vector<uint64_t>& first,
                 std::vector<uint64_t>& count) {
    if (!c->have_scan || !c->hcache_valid || c->rx) return false;
    frames.swap(c->hcache);
    first.swap(c->hfirst);
    count.swap(c->hcount);
    c->hcache.clear();
    c->hcache_valid = false;
    c->have_scan = false;
    return true;
}

// True when [p, p+len) lies in registered pinned memory (hvws_rx_reads can take it).
bool is_pinned(const void* p, uint64_t len) { return pinned_dev(p, len) != nullptr; }

// Per-thread pinned staging for batched host entry points.
char* pinned_stage(uint64_t bytes) {
    hvws_ctx* c = thread_ctx();
    if (hipSetDevice(c->device) != hipSuccess || c->h_feed.ensure(bytes + 64) != hipSuccess)
        fatal("pinned staging allocation");
    return c->h_feed.as<char>();
}

// XOR `n` host bytes at src into dst with key/phase on the GPU.
void gpu_xor_host(char* dst, const char* src, size_t n, uint32_t key, uint32_t phase) {
    if (n == 0) return;
    hvws_ctx* c = thread_ctx();
    if (door_xor(c, dst, src, n, key, phase)) return;   // no HIP call on the worker's path
    if (hipSetDevice(c->device) != hipSuccess) fatal("hipSetDevice");
    if (c->xor_stage.ensure(n + 64) != hipSuccess) fatal("device staging allocation");
    uint8_t* d = c->xor_stage.as<uint8_t>();
    if (hipMemcpyAsync(d, src, n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        launch_xor_span(d, n, key, phase, c->stream) != hipSuccess ||
        hipMemcpyAsync(dst, d, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        set_err(HVWS_EHIP, "xor span failed");
        fatal("websocket_decode on the GPU");
    }
}

// One-segment batch from host memory for the streaming drop-in.
// Returns frames and the carry-out (WebSocketParser semantics).
void gpu_feed(char* buf, size_t len, const websocket_parser& carry, bool unmask, std::vector<hvws_frame>& frames,
              websocket_parser& carry_out, int& started) {
    hvws_ctx* c = thread_ctx();
    if (door_feed(c, buf, len, carry, unmask, frames, carry_out, started)) return;   // no HIP call there
    if (hipSetDevice(c->device) != hipSuccess) fatal("hipSetDevice");
    hvws_segment seg = {0, (uint64_t)len};
    websocket_parser cin;
    copy_parser(cin, carry);
    if (hvws_rx_batch(c, (uint8_t*)buf, len, &seg, &cin, 1, unmask ? 1 : 0) != HVWS_OK) fatal("hvws_rx_batch");
    const int64_t n = hvws_frame_count(c);
    frames.resize((size_t)n);
    if (n > 0 && hvws_get_frames(c, frames.data(), 0, (uint64_t)n) != HVWS_OK) fatal("hvws_get_frames");
    int st = 0;
    if (hvws_get_carry(c, nullptr, &st) != HVWS_OK) fatal("hvws_get_carry");
    copy_parser(carry_out, cin);
    started = st;
}

}  // namespace hvws
