// hvws_internal.h -- shared between the HIP kernels and the host engine.
#pragma once

#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <stddef.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <functional>

#include "websocket_parser.h"

struct hvws_ctx;

namespace hvws {

// $HVWS_EXPERIMENT="name=value,name=value": the A/B switches of the on-device
// sweeps (DESIGN.md sec. 9 lists them).  The text of `name`'s value (up to
// the next ','; atoi / strtoull stop there) or nullptr; read from the
// environment on every call (callers that keep a value cache it themselves).
inline const char* experiment(const char* name) {
    const char* e = getenv("HVWS_EXPERIMENT");
    if (!e) return nullptr;
    const size_t n = strlen(name);
    for (const char* p = e; p && *p; p = strchr(p, ',') ? strchr(p, ',') + 1 : nullptr)
        if (!strncmp(p, name, n) && p[n] == '=') return p + n + 1;
    return nullptr;
}

// With validation on, the state of a header split across reads lives in the
// padding byte after websocket_parser.mask_offset (the reference never reads
// it).  Copies of the struct inside the library go through memcpy: a struct
// assignment may copy member by member and drop the padding.
constexpr size_t kViolByte = offsetof(websocket_parser, mask_offset) + 1;
static_assert(offsetof(websocket_parser, length) > kViolByte, "validation byte must be padding");
inline void copy_parser(websocket_parser& dst, const websocket_parser& src) { memcpy(&dst, &src, sizeof dst); }

// Parser states (reference enum at http/websocket_parser.c:34-40).
enum : uint32_t { S_START = 0, S_HEAD = 1, S_LENGTH = 2, S_MASK = 3, S_BODY = 4 };
enum : uint32_t { F_OPMASK = 0x0Fu, F_FIN = 0x10u, F_MASK = 0x20u };
enum : uint32_t {
    I_HDR = 1u << 10, I_BODY = 1u << 11, I_END = 1u << 12, I_START = 1u << 13, I_INVALID = 1u << 14
};
// Optional protocol validation (RFC 6455 sec. 5.1-5.5; the reference checks
// none of these).  Violation classes, reported in info bits
// I_VSHIFT.. of a frame whose header completes, only for classes enabled in
// the context's validation mask (0 = off = reference behaviour).
enum : uint32_t {
    V_RSV = 1u,        // RSV1-3 set with no extension negotiated
    V_OPCODE = 2u,     // reserved opcode 3-7 / 0xB-0xF
    V_CONTROL = 4u,    // control frame fragmented (FIN = 0) or longer than 125 bytes
    V_LEN64 = 8u,      // 64-bit length with the most significant bit set
    V_NONMIN = 16u,    // length not in its minimal encoding
    V_UNMASKED = 32u,  // client-to-server frame without a mask
    V_ALL = 63u,
    V_ENC_SHIFT = 6u,  // (carry only) 2-bit length encoding of a partial header: 1 = 16-bit, 2 = 64-bit
    I_VSHIFT = 16u
};

// Device-side carry (the websocket_parser fields the walk needs), 48 bytes.
struct dcarry {
    uint32_t state;
    uint32_t flags;
    uint32_t mask;         // mask[0] in bits 0-7
    uint32_t mask_offset;
    uint64_t length;
    uint64_t require;
    uint64_t offset;
    uint32_t started;      // first header byte of the pending frame was in this segment
    uint32_t viol;         // V_* bits (+ encoding) of the partial header, for validation
};

// Per-segment state between the discovery kernels (k_head -> k_verify -> k_walk).
struct dmid {
    dcarry   st;       // parser state after the carried-in frame
    uint64_t pos;      // segment offset of the first whole frame
    uint64_t stride;   // its size (speculation stride), 0 if none
    uint64_t n_a;      // frames recorded before pos (0 or 1)
    uint64_t pad;
};

struct dseg {
    uint64_t off;
    uint64_t len;
};

// Frame table, structure of arrays in HBM (one entry per frame per batch).
struct dframes {
    int64_t*  hdr_off;   // absolute, -1 = header began in an earlier batch
    uint64_t* pay_off;   // absolute
    uint64_t* pay_len;
    uint64_t* length;
    uint32_t* key;       // raw key
    uint32_t* keyrot;    // key rotated for 4-byte aligned words (0 if not masked)
    uint32_t* info;
    uint64_t  cap;       // records the arrays hold; EMIT drops records beyond it (counts stay exact)
};

// One frame record as handed to the host (layout of hvws_frame, 40 bytes).
struct drec {
    int64_t  hdr_off;
    uint64_t pay_off;
    uint64_t pay_len;
    uint64_t length;
    uint32_t key;
    uint32_t info;
};

// Per-segment result of the small-batch kernel, written to pinned host memory.
struct dsmall_out {
    uint64_t first;   // index of the segment's first record in the host record area
    uint64_t count;
    dcarry   st;      // carry out
};

constexpr int SCAN_THREADS = 256;           // 4 waves, one segment per wave
constexpr int SCAN_U = 4;                   // predicted frames per lane per round
constexpr int UNMASK_MAXF = 512;            // frames staged in LDS per tile

// Result of k_spec_check, written by the device into pinned host memory.
struct dspec_status {
    uint64_t seq;     // scan sequence number it belongs to
    uint64_t total;   // records of the batch (sum of the true counts)
    uint32_t flags;   // SPEC_*
    uint32_t pad;
    uint64_t max_seg_count;   // largest segment count: sizes the next SLACK table
    uint64_t long_run_seen;   // some segment had >= spec_min predicted frames (the next pass's verify hint)
    uint64_t tseq;    // seq again, published after the scan's last kernel (tile index complete)
    uint64_t run_seq;      // RUN: the step whose repair pass published last (k_run_fix)
    uint64_t run_failed;   // ... and its failed segments
};
static_assert(sizeof(dspec_status) == 64 && offsetof(dspec_status, seq) == 0 && offsetof(dspec_status, total) == 8 &&
                  offsetof(dspec_status, flags) == 16 && offsetof(dspec_status, max_seg_count) == 24 &&
                  offsetof(dspec_status, long_run_seen) == 32 && offsetof(dspec_status, tseq) == 40 &&
                  offsetof(dspec_status, run_seq) == 48 && offsetof(dspec_status, run_failed) == 56,
              "dspec_status layout: the host polls these words, the kernels store them");
enum : uint32_t {
    SPEC_MATCH = 1u,   // every segment's record count equals k_head's estimate
    SPEC_OK = 2u,      // SCAN_SPEC: the speculative table is the exact table (match and within capacity)
    SPEC_ERR = 4u      // one-launch scan: a grid barrier timed out (results void)
};

struct sieve_bufs;

// RUN path (round 5): a batch whose segments each hold one run of equal
// frames (the last check saw uniform counts) is unmasked from per-segment
// descriptors alone -- no per-frame records, no second pass over the header
// lines.  k_head writes the descriptor (the carried-in frame and the frame cut
// by the segment end exactly, the run in between as a hypothesis: the first
// whole frame's size repeated); k_unmask_run parses every run header from
// the tile bytes it loads anyway, checks it against the hypothesis and takes
// its key from it; k_run_fix, queued behind on the same stream, undoes and
// redoes exactly any segment whose hypothesis failed, so work queued after a
// step always sees the reference's bytes.  Frame records are built on demand
// (an exact scan of the unchanged headers) when a reader asks for them.
struct drun {
    uint64_t seg_lo, seg_hi;   // the segment's absolute byte range
    uint64_t p0;               // absolute offset of the run's first header
    uint64_t stride;           // bytes per frame of the run (0: no run)
    uint64_t len;              // payload bytes per frame of the run
    double   inv;              // 1 / stride
    uint32_t cnt, hlen;        // frames in the run, header bytes of each
    uint32_t masked, flags;    // run frames carry a key (the first's mask bit); RUN_*
    uint64_t a_off, a_end;     // carried-in frame's payload piece [a_off, a_end), absolute
    uint64_t t_off, t_end;     // payload piece of the frame cut by the segment end
    uint32_t a_kw, t_kw;       // their key words for 4-byte aligned words (0: nothing to XOR)
    uint64_t pad;
    dcarry   cin;              // the segment's carry-in (the repair's exact path; the shared
                               // carry table belongs to the next scan by then)
};
static_assert(sizeof(drun) == 160, "drun layout");
// Per unmask tile (64 bytes, k_run_tiles): the first segment meeting the
// tile (s0, nseg if none) and the last (s1), and s0's run as it meets the
// tile, tile-relative: its first run frame's header h0 (>= -S), the run
// frames meeting the tile (nj; 0 if s0 is left to the repair), k0 -- the key
// of the run frame begun before the tile (its header read beside the previous
// unmask) -- and the carried-in / cut frame's payload pieces clipped to the
// tile.  A tile of one segment needs no other load before its unmask.
struct dtrun {
    uint32_t s0, s1, k0;
    int32_t  h0;
    uint32_t nj, S, len, hm;    // run frames meeting the tile, stride, payload bytes, header bytes | masked << 8
    int32_t  a_lo, a_hi, t_lo, t_hi;
    uint32_t a_kw, t_kw;        // 0: no piece
    uint32_t pad[2];
};
static_assert(sizeof(dtrun) == 64, "dtrun layout");
enum : uint32_t { RUN_BAD = 1u };   // the segment is not one run (k_head saw it): exact repair only
constexpr uint64_t RUN_MAX_FRAME = 8192;   // frames at most this size take the RUN path (bigger: SPEC)
constexpr uint64_t RUN_MIN_SEG = 65536;    // and segments of at least this size on average
// k_head<false> writes runs[s] when given; k_run_tiles: trun[t] for every
// unmask tile (t < ntiles, dtrun); fail[s] is segment
// s's failure word (zeroed by k_head; k_run_tiles sets bit 2 for a segment
// k_unmask_run leaves to the repair), fail[nseg .. nseg + 2] the batch's
// (any failed, failed count, repair workgroups done), zero between RUN steps
// (the repair clears them all; the host zeroes a new array).
hipError_t launch_run_tiles(const uint8_t* rx, uint64_t rx_len, const dseg* segs, uint32_t nseg, const drun* runs,
                            dtrun* trun, uint64_t ntiles, uint64_t tile, uint32_t* fail, hipStream_t st);
// The RUN unmask (RUN_TILE bytes per tile, the tiles k_run_tiles described)
// and its repair pass; the timing events ride on the unmask's first dispatch
// (start) and the repair's (stop).  The repair publishes (seq, failed
// segments) to status->run_seq / run_failed when it is done.
constexpr uint64_t RUN_TILE = 16384;   // 256 threads x 4 chunks of 16 B
const char* run_kernel_name();
hipError_t launch_unmask_run(uint8_t* rx, uint64_t rx_len, const drun* runs, const dtrun* trun, uint32_t nseg,
                             uint32_t* fail, dspec_status* status, uint64_t seq, hipStream_t st, hipEvent_t ev_start,
                             hipEvent_t ev_stop);
constexpr uint64_t RUN_FAST_STRIDE = 1u << 20;   // run strides up to this take k_unmask_run's one-segment path

struct scan_scratch {   // host-side bundle for launch_scan: per-segment arrays (nseg entries) + one total
    dmid*     mid = nullptr;
    uint64_t* npred = nullptr;
    uint64_t* pbase = nullptr;
    uint64_t* first_fail = nullptr;
    uint64_t* last_masked = nullptr;   // 1 + index of the last masked verified frame, 0 none
    uint64_t* total_pred = nullptr;
    uint64_t* est = nullptr;           // records k_head predicts per segment (uniform-stride hypothesis)
    // Zero-copy upload: when src_segs is set, the first k_head of the scan
    // reads the segment and carry tables from these (device-mapped pinned
    // host) arrays and writes the device tables the later kernels read.
    const dseg*   src_segs = nullptr;
    const dcarry* src_carry = nullptr;
    dseg*         segs_w = nullptr;
    dcarry*       carry_w = nullptr;
    dspec_status* status = nullptr;    // device-mapped pinned host
    uint64_t      seq = 0;
    const sieve_bufs* sieve = nullptr; // SINGLE / its re-EMIT: frame sieve buffers, nullptr = no sieve
    dframes   slack{};                 // SLACK: scratch table
    uint64_t  slack_cap = 0;           // SLACK: records per segment region at most
    uint64_t* bases_x = nullptr;       // SLACK: exact bases (nseg)
    uint64_t* est_u = nullptr;         // SLACK: uniform-stride estimates (nseg), for SPEC_MATCH
    uint32_t  no_verify = 0;           // SPEC/SLACK: head + walk only (no k_verify pair, no k_head<true>)
    drun*     runs = nullptr;          // RUN: k_head writes each segment's run descriptor
    uint32_t* run_fail = nullptr;      // RUN: per-segment failure words + the batch's, zeroed by k_head / k_run_tiles
    dtrun*    run_trun = nullptr;      // RUN: per unmask tile (run_ntiles entries)
    uint64_t  run_ntiles = 0, run_tile = 0;
};

// Bijective XCD-contiguous tile order: the dispatcher deals blocks b, b+8,
// b+16, ... to one XCD; map them to adjacent tiles so each XCD's L2 and
// memory channels see one contiguous range.
__device__ __forceinline__ uint64_t xcd_tile(uint64_t b, uint64_t ntiles) {
    const uint64_t q = ntiles >> 3, r = ntiles & 7u, x = b & 7u, i = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// Workgroup b -> tile, runs of g adjacent tiles per XCD: within each window
// of 8 g tiles, XCD x (= b mod 8, the hardware's round-robin placement) takes
// tiles x g .. x g + g - 1, in order.  Neighbouring tiles that share a cache
// line (a payload span's boundary line, a line of the per-frame tables) then
// meet in one L2 instead of being fetched from memory by two XCDs, while the
// eight XCDs still stream through the same window of memory (the whole-range
// XCD order of xcd_tile halved k_build's rate).  A bijection on
// [0, ntiles): the last partial window keeps the linear order.
__device__ __forceinline__ uint64_t xcd_group_tile(uint64_t b, uint64_t ntiles, uint32_t g) {
    const uint64_t win = 8ull * g, full = ntiles - ntiles % win;
    if (g <= 1 || b >= full) return b;
    const uint64_t w = b / win, r = b % win;
    return w * win + (r & 7u) * g + (r >> 3);
}

// Frame sieve (hvws_sieve.hip): parallel discovery of one long mixed-size
// stream.  State of the current scan, device side.
struct dsieve {
    uint64_t active;        // this scan's one segment is sieved
    uint64_t use;           // k_walk resumes at pend with npath chain frames recorded
    uint64_t pend;          // segment offset where the exact walk resumes
    uint64_t last;          // 1 + segment offset of the chain's last frame
    uint64_t last_masked;   // 1 + segment offset of the chain's last masked frame
    uint64_t npath;         // frames on the chain
    uint64_t pad[2];
};

// Device buffers of the sieve (per context; scans run in order on one stream).
struct sieve_bufs {
    dsieve*   state;
    uint64_t* tcount;    // per 8 KiB tile: survivors        (sieve_tiles_max entries)
    uint64_t* tbase;     // exclusive scan of tcount          (sieve_tiles_max)
    uint32_t* slot;      // first survivors of each tile      (sieve_slot_words)
    uint32_t* pool;      // survivors of tiles with more      (capS)
    uint64_t* pool_n;    // pool entries used
    uint64_t* keep;      // 1 = survivor after HBM verification (capS)
    uint64_t* kbase;     // exclusive scan of keep            (capS)
    uint64_t* Spre;      // survivors before HBM verification (capS)
    uint64_t* m_pre;     // entries of Spre
    uint64_t* S;         // survivor segment offsets, sorted  (capC)
    uint32_t* J0;        // successor / doubling tables       (capC each)
    uint32_t* J1;
    uint64_t* mark;      // 1 = on the chain                  (capC)
    uint32_t* hops;      // whole frames from a node to its successor (capC)
    uint64_t* rank;      // exclusive scan of mark * hops     (capC)
    uint64_t* m_total;   // survivors
    uint64_t* npath;     // chain frames
    uint64_t* tmp;       // scan scratch (>= 4 * ceil(max(capS, tiles) / 1024) + 64 words)
    uint64_t  capS;      // entries before verification, < 2^32
    uint64_t  capC;      // survivors / chain nodes, <= capS
    uint32_t  rt, wt;    // windows: the first wt of every rt tiles are sieved (rt == wt: every tile)
    uint64_t* scr;       // windowed: each node's first 2^lgP frame offsets (capC << lgP), or nullptr
    uint32_t  lgP;
};
uint64_t sieve_tiles_max(uint64_t rx_len);
uint64_t sieve_slot_words(uint64_t rx_len);
uint64_t sieve_min();                  // bytes after the first whole frame from which a mixed stream is sieved
uint64_t set_sieve_min(uint64_t v);    // 0 = default; returns the previous value
uint64_t sieve_generation();           // bumped by set_sieve_min (contexts forget their sieve history)
// Window geometry for a one-segment scan of rx_len bytes whose last exact
// count was nframes (0: unknown -> every tile): rt, wt in tiles.
void sieve_geometry(uint64_t rx_len, uint64_t nframes, uint32_t& rt, uint32_t& wt);
void set_sieve_windows(uint64_t hops, uint64_t window, uint64_t prev[2]);   // bumps sieve_generation()
uint64_t sieve_hops();                 // frames per region the window geometry aims at (0: windows off)
hipError_t launch_sieve(const uint8_t* rx, uint64_t rx_len, const dseg* segs, const dmid* mid, const uint64_t* npred,
                        const sieve_bufs& b, hipStream_t st);
hipError_t launch_sieve_emit(const uint8_t* rx, uint64_t rx_len, const dseg* segs, const dmid* mid,
                             const sieve_bufs& b, dframes fr, uint32_t vmask, hipStream_t st);

// Kernel launchers (hvws_kernels.hip).
// COUNT pass (emit=false): counts[], bases[] (exclusive scan) and *total.
// EMIT pass: frame table at bases[], carry_out[].
// SINGLE (one segment, base 0 known): COUNT's speculation only, then EMIT,
// which also writes counts[] -- the serial walk of a mixed-size stream runs
// once instead of twice.
// SPEC (several segments, frame table of known capacity): EMIT at bases
// taken from k_head's per-segment estimates, then k_spec_check compares the
// true counts with them -- equal everywhere means the table is exact, so a
// uniform batch is discovered with one walk and no host round trip before
// EMIT; otherwise *total is zeroed (the tile kernels and k_unmask then do
// nothing) and the host re-runs COUNT + EMIT.  COUNT also runs the check,
// to tell the host whether the next batch is worth speculating on.
// SLACK (several segments of mixed sizes): one EMIT walk into per-segment
// regions of a scratch table (sized by each segment's record bound, capped at
// slack_cap), then a device check that every segment fit and a compaction into
// the frame table at the exact bases; a segment that did not fit zeroes *total
// and the host re-scans COUNT + EMIT.
// RUN: k_head writing run descriptors (no est, no walk) + the tile-segment index.
enum scan_pass { SCAN_COUNT = 0, SCAN_EMIT = 1, SCAN_SINGLE = 2, SCAN_SPEC = 3, SCAN_SLACK = 4, SCAN_RUN = 5 };
hipError_t launch_scan(int pass, const uint8_t* rx, uint64_t rx_len, const dseg* segs, uint32_t nseg,
                       const dcarry* carry_in, dcarry* carry_out, uint64_t* counts, uint64_t* bases,
                       uint64_t* total, scan_scratch sc, dframes fr, uint32_t vmask, hipStream_t st);
hipError_t launch_offsets(const uint64_t* counts, uint64_t* bases, uint32_t nseg, uint64_t* total,
                          hipStream_t st);
// status->tseq = seq (system-scope release), after every earlier kernel of the stream:
// the host sees that the scan's tables are complete without a stream event.
hipError_t launch_publish_tiles(dspec_status* status, uint64_t seq, hipStream_t st);
// *total > cap: *total = 0; publishes the count to status (SPEC_OK if within cap).
hipError_t launch_cap_check(uint64_t* total, uint64_t cap, dspec_status* status, uint64_t seq, hipStream_t st);
hipError_t launch_ends_check(const uint64_t* off, const uint64_t* len, const uint64_t* nfr_dev,
                             unsigned long long* bad, hipStream_t st);
hipError_t launch_tile_index(const uint64_t* off, const uint64_t* len, uint64_t nfr, const uint64_t* nfr_dev,
                             uint32_t* tile_first, uint64_t ntiles, uint64_t tile, hipStream_t st);
// Tile index marks: a tile no frame's scatter reached (k_tile_fixup searches
// it); a frame scatters itself into at most TILE_SPAN_MAX tiles.
constexpr uint32_t TILE_MARK = 0xFFFFFFFFu;
constexpr uint64_t TILE_SPAN_MAX = 64;
// k_tile_fixup alone (tile_first already scattered).
hipError_t launch_tile_fixup(const uint64_t* off, const uint64_t* len, uint64_t nfr, uint32_t* tile_first,
                             uint64_t ntiles, uint64_t tile, hipStream_t st);
// Small batches, whole path in one launch (one wave per segment): records
// into slots[slot_base[s]..], then compacted into h_rec (pinned host) when
// they fit h_rec_cap; results into h_out[s]; unmasked chunks into h_rx
// (pinned host, same layout as rx).  *rec_total (device) must equal rec_base
// on entry and advances by the records written.  stage_lds != 0: each segment
// is staged in stage_lds bytes of LDS (>= its 16-aligned span + 16); rx,
// segs, carry_in and slot_base may then be pinned host memory read in place
// (zero-copy).
constexpr uint64_t kStageSegment = 32ull << 10;   // largest segment k_small stages in LDS
constexpr uint64_t kZcBatch = 1ull << 20;         // largest batch sent zero-copy
hipError_t launch_small(const uint8_t* rx, uint64_t rx_len, const dseg* segs, const dcarry* carry_in, uint32_t nseg,
                        const uint64_t* slot_base, drec* slots, unsigned long long* rec_total, uint64_t rec_base,
                        drec* h_rec, uint64_t h_rec_cap, dsmall_out* h_out, uint8_t* h_rx, int unmask, uint32_t vmask,
                        uint32_t stage_lds, uint64_t* h_done, uint64_t seq, hipStream_t st,
                        hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// Resident small-path worker ("door", k_door): one workgroup that stays on
// the device between calls and takes one request at a time from a mailbox in
// fine-grained pinned host memory, so a reference-API call (FeedRecvData,
// websocket_parser_execute, websocket_decode, a masked websocket_build_frame)
// pays neither a launch nor a dispatch.  The host writes the request fields,
// then `seq` (release); the worker serves it and publishes `done = seq`
// (system-scope release) after its results.  A worker idle for idle_ticks of
// the 100 MHz realtime clock parks itself (alive = 0, after one last look at
// seq) and the next request relaunches it.  Every launch carries an epoch;
// a worker's last store before it returns is `exited = epoch`, and the host
// takes that word -- not the stream's status -- as the sign that the worker
// has ended ("Resident worker").
enum : uint32_t { DOOR_FEED = 1u, DOOR_XOR = 2u, DOOR_EXIT = 3u };
constexpr uint32_t kDoorThreads = 512;              // 8 waves: staging and XOR in parallel, walk on wave 0
constexpr uint64_t kDoorMax = 32ull << 10;          // largest request (bytes)
constexpr uint64_t kDoorRecords = kDoorMax / 2 + 3; // records a kDoorMax segment can hold
struct ddoor {
    // host -> device (written before seq)
    uint64_t seq;
    uint32_t op;
    uint32_t unmask;
    uint64_t len;
    uint32_t vmask;
    uint32_t key;       // DOOR_XOR: mask word (mask[0] in bits 0-7)
    uint32_t phase;     // DOOR_XOR: mask_offset of the first byte
    uint32_t pad0;
    dcarry   carry;     // DOOR_FEED: carry in
    uint64_t pad1[4];
    uint64_t seq_tail;  // seq again, written with the fields (before seq): the worker reads the
                        // whole block with its poll and takes it when both copies agree
    // device -> host (own cache lines; `done` written last)
    uint64_t done;      // seq of the last request served
    uint64_t alive;     // 1 while a worker runs (0 once it parked)
    uint64_t count;     // DOOR_FEED: records written
    uint64_t served;    // requests served by this worker (diagnostic)
    dcarry   out;       // DOOR_FEED: carry out
    uint64_t exited;    // epoch of the last worker that has ended (its last store before it returns)
    uint64_t pad2[1];
    // realtime-clock stamps of the last request (100 MHz): seen, staged,
    // walked, xored, stored (before the release); read by hvws_door_stamps'
    // diagnostics (scripts/probe/door_phases.py)
    uint64_t stamp[12];   // [6]: the previous request's release, ticks; [8..10]: door_walk's chase, parse, tail ends
};
static_assert(sizeof(dcarry) == 48, "dcarry layout");
static_assert(offsetof(ddoor, done) == 128, "ddoor: device fields on their own lines");
static_assert(offsetof(ddoor, seq_tail) == 120, "k_door reads seq_tail as the last 8 bytes of the request block");
static_assert(offsetof(ddoor, carry) == 40 && offsetof(ddoor, len) == 16 && offsetof(ddoor, vmask) == 24,
              "k_door reads the request as words 1-10");
// data areas: kDoorMax + 256 bytes (256-aligned); h_rec: kDoorRecords records
// (pinned); d_slot: kDoorRecords records (device) for records past the LDS area.
// req: the request block (words 0-15 of a ddoor) -- fine-grained device
// memory the host writes through the PCIe BAR, or the pinned box itself;
// din: the request's bytes (same choice); dout: results (pinned host; may equal
// din when both are the pinned area).
// k_door's kernel arguments, as an AQL dispatch of it reads them (the
// kernel's explicit arguments in order; it uses no hidden ones).
struct door_args {
    const ddoor* req;
    ddoor* box;
    const uint8_t* din;
    uint8_t* dout;
    drec* h_rec;
    drec* d_slot;
    uint64_t idle_ticks, first_seq, epoch;
    uint32_t flags;
};
uint32_t door_flags();                      // k_door's flags ($HVWS_EXPERIMENT door_stamps)
hipError_t door_anchor(void** dev_addr);    // a device symbol of k_door's code object (loads it on the device)
const char* door_kernel_symbol_prefix();    // k_door's symbol name, up to its argument types

// The worker's own HSA queue (hvws_doorq.cpp): k_door dispatched by one AQL
// packet per launch; `done` (its completion signal) reaches 0 when the launch
// has ended; destroyed only then.
struct door_queue {
    hsa_queue_t* q = nullptr;
    hsa_signal_t done{0};
    hsa_agent_t agent{0};
    uint64_t object = 0;                   // k_door's kernel descriptor
    uint32_t group = 0, priv = 0, kernarg_size = 0;
    void* kernarg = nullptr;               // pinned host
    void* kernarg_dev = nullptr;
    int device = -1;
    bool at_exit = false;                  // destroyed from the exit handler: no HIP call
    std::atomic<int> error{0};             // queue error reported by the runtime (hsa_status_t)
};
int  door_queue_create(int device, door_queue** out);
int  door_queue_launch(door_queue* q, const void* args, uint32_t nargs);
bool door_queue_idle(door_queue* q);     // the last launch has ended (or none was made)
int  door_queue_error(door_queue* q);    // 0, or the queue's error status
const char* door_queue_why();            // what the last failing door_queue_* call of this thread hit
void door_queue_destroy(door_queue* q);  // only when idle

// Host copy pool (hvws_hostpool.cpp): fn(i) for i in [0, n) on up to
// copy_width() threads (the caller included; serial when another caller
// holds the pool); par_memcpy splits copies of >= kParCopyMin bytes.
constexpr uint64_t kParCopyMin = 1ull << 20;
int copy_width();
void par_for(int n, const std::function<void(int)>& fn);
void par_memcpy(void* dst, const void* src, uint64_t n);
// Batched handshake digest (hvws_keys.hip): accept[32*i..] = base64(SHA-1(key_i + GUID)), 28 chars + 4 zero bytes.
hipError_t launch_encode_keys(const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len, uint64_t n,
                              uint8_t* accept, hipStream_t st);
// UTF-8 validation of text messages (hvws_utf8.hip; include/hvws.h has the
// state machine, the transition words and the fold rules).  Reads rx and the
// frame table only.  nfr_dev: the batch's record count on the device, clamped
// to cap (the entries words / flags hold).  tile_first: ntiles + 1 entries of
// launch_tile_index at U8_TILE.  flags: one word per record, all zero on
// entry (the caller zeroes a new array), set by k_u8_tiles where a payload's
// interior (bytes 3 ..) breaks a character and cleared again by k_u8_words.
// meta[0] receives the clamped record count.  Then the per-segment fold:
// state_in (nullptr: all 0) -> state_out, bad.
constexpr uint64_t U8_TILE = 16384;   // 256 threads x 4 chunks of 16 B
constexpr uint32_t U8_ACCEPT = 0u, U8_REJECT = 15u, U8_TEXT_OPEN = 16u, U8_IDENTITY = 0x76543210u;
hipError_t launch_utf8(const uint8_t* rx, uint64_t rx_len, const uint64_t* pay_off, const uint64_t* pay_len,
                       const uint32_t* keyrot, const uint32_t* info, const uint64_t* nfr_dev, uint64_t cap,
                       const uint32_t* tile_first, uint64_t ntiles, int masked, uint32_t* flags, uint32_t* words,
                       uint64_t* meta, const uint64_t* counts, const uint64_t* bases, uint32_t nseg,
                       const uint32_t* state_in, uint32_t* state_out, uint64_t* bad, hipStream_t st);
// Message reassembly (hvws_msg.hip; include/hvws.h has the rule, the layout
// and the carry).  dmsg_state / dmsg mirror hvws_msg_state / hvws_msg.
struct dmsg_state {
    uint64_t pending;
    uint32_t opcode, open;
};
struct dmsg {
    uint64_t off, len, total, rec;
    uint32_t seg, info;
};
struct drfc_state {   // mirrors hvws_rfc_state
    dmsg_state data, ctl;
    uint64_t data_off, ctl_off;
};
enum : uint32_t { M_END = 1u << 4, M_CONT = 1u << 5, M_CTL = 1u << 6 };
constexpr uint64_t MSG_TILE = 16384;   // output bytes of k_msg_gather's largest tile (every geometry's divides it)
// k_msg_gather geometry for a batch of rx_len bytes in at most cap records
// ($HVWS_EXPERIMENT msg, else by the mean bytes per record) and its tile
int msg_variant(uint64_t rx_len, uint64_t cap);
uint64_t msg_gather_tile(int g);
uint64_t msg_scratch_bytes(uint64_t cap);
// The table pass, reading the frame table only.  nfr_dev / cap as for
// launch_utf8; scratch: msg_scratch_bytes(cap); out_off: cap words; msgs:
// cap + 1 entries; state_in (device, nullptr: all fresh) -> state_out;
// meta[0..2] = records, payload bytes, pieces.
hipError_t launch_msg_table(const uint64_t* pay_len, const uint32_t* info, const uint64_t* nfr_dev, uint64_t cap,
                            const uint64_t* counts, const uint64_t* bases, uint32_t nseg, const dmsg_state* state_in,
                            void* scratch, uint64_t* out_off, dmsg* msgs, uint64_t* seg_first, uint64_t* seg_count,
                            dmsg_state* state_out, uint64_t* meta, hipStream_t st);
// The gather, geometry g: tile_first is launch_tile_index over (out_off,
// pay_len, meta) at msg_gather_tile(g) with ntiles tiles (ntiles tiles hold
// the payload bytes; tiles beyond them do nothing).  Writes
// out[0 .. min(meta[1], out_cap)) only.
hipError_t launch_msg_gather(int g, const uint8_t* rx, uint64_t rx_len, const uint64_t* pay_off, const uint64_t* pay_len,
                             const uint32_t* keyrot, const uint64_t* out_off, const uint32_t* tile_first,
                             uint64_t ntiles, const uint64_t* meta, int masked, uint8_t* out, uint64_t out_cap,
                             hipStream_t st);
// The joined form (hvws_messages_joined): both passes over rows -- per segment
// its carried span, then its records; cap + nseg of them.  len / src / key /
// info: the row table k_join_rows writes; prow: each piece's last row (rows + 1
// words).  All device memory.
struct msg_rows {
    uint64_t* len;
    uint64_t* src;
    uint32_t* key;
    uint32_t* info;
    uint64_t* prow;
};
// launch_msg_table over rows: fr's pay_off / pay_len / keyrot / info are read;
// scratch: msg_scratch_bytes(cap + nseg); out_off: cap + nseg words; msgs:
// cap + nseg + 1 entries; state_in and prev_off (device, nseg entries) may be
// null when nothing is pending; carry_off: nseg words; meta[0..2] = rows, bytes
// (carried and payload), pieces.  nseg > 0.
hipError_t launch_msg_table_joined(const dframes& fr, int masked, const uint64_t* nfr_dev, uint64_t cap,
                                   const uint64_t* counts, const uint64_t* bases, uint32_t nseg,
                                   const dmsg_state* state_in, const uint64_t* prev_off, void* scratch,
                                   const msg_rows& rows, uint64_t* out_off, dmsg* msgs, uint64_t* seg_first,
                                   uint64_t* seg_count, dmsg_state* state_out, uint64_t* carry_off, uint64_t* meta,
                                   hipStream_t st);
// launch_msg_gather over rows: tile_first is launch_tile_index over (out_off,
// rows.len, meta).  No read leaves [rx, rx + rx_len) or [prev, prev + prev_len).
hipError_t launch_msg_gather_joined(int g, const uint8_t* rx, uint64_t rx_len, const uint8_t* prev, uint64_t prev_len,
                                    const msg_rows& rows, const uint64_t* out_off, const uint32_t* tile_first,
                                    uint64_t ntiles, const uint64_t* meta, int masked, uint8_t* out, uint64_t out_cap,
                                    hipStream_t st);
// The RFC form (hvws_messages_rfc): rows as in the joined form, scattered into
// output order -- per connection its data carried row and data records, then
// its control carried row and control records: cap + 2 nseg of them, two
// virtual connections per connection.  rec: each row's frame-table index;
// vbase / vcnt: each virtual connection's carried row and record count
// (2 nseg words each).
struct rfc_rows {
    uint64_t* rec;
    uint64_t* vbase;
    uint64_t* vcnt;
};
uint64_t msg_cls_bytes(uint64_t cap);
// launch_msg_table_joined over those rows.  scratch: msg_scratch_bytes(cap +
// 2 nseg); cls_scratch: msg_cls_bytes(cap); row tables and out_off: cap + 2 nseg
// entries; msgs: one more; vstate_in / voff (device, 2 nseg entries: 2s data,
// 2s + 1 control) may be null when nothing is pending; state_out: nseg entries.
// launch_msg_gather_joined and the tile index then run over rows unchanged.
hipError_t launch_msg_table_rfc(const dframes& fr, int masked, const uint64_t* nfr_dev, uint64_t cap,
                                const uint64_t* bases, uint32_t nseg, const dmsg_state* vstate_in,
                                const uint64_t* voff, void* scratch, void* cls_scratch, const msg_rows& rows,
                                const rfc_rows& rr, uint64_t* out_off, dmsg* msgs, uint64_t* seg_first,
                                uint64_t* seg_count, drfc_state* state_out, uint64_t* meta, hipStream_t st);
// Batched send and server replies (hvws_send.hip; include/hvws.h has both
// contracts).  dtxmsg mirrors hvws_tx_msg.
struct dtxmsg {
    uint64_t off, len;
    uint32_t flags, key;
};
enum : uint32_t { R_PONG = 1u, R_CLOSE = 2u, R_ECHO = 4u, RF_CLOSED = 1u, RF_DEFERRED = 2u, RF_FAILED = 4u };
uint64_t send_scratch_bytes(uint64_t n);
// The message pass over msgs[0 .. min(*n_dev, n)) (n_dev may be null), F bytes
// per fragment: scratch (send_scratch_bytes(n)) keeps each message's frames and
// output bytes before it; first: n + 1 words, each message's first frame;
// msg_off: the same in output bytes (optional); meta (zeroed by the caller):
// [0..3] = frames, output bytes, bad messages, effective count, [4] = messages
// breaking the uniform layout, [5..7] = off[0], off[1] - off[0], len[0].
hipError_t launch_send_table(const dtxmsg* msgs, uint64_t n, const uint64_t* n_dev, uint64_t plen, uint64_t F,
                             int masked, void* scratch, uint64_t* first, uint64_t* msg_off, uint64_t* meta,
                             hipStream_t st);
// One thread per frame (nframes = meta[0], read by the host): the rows
// launch_tx_index / launch_build take.
hipError_t launch_send_expand(const dtxmsg* msgs, const void* scratch, const uint64_t* first, const uint64_t* meta,
                              uint64_t nframes, uint64_t F, int masked, uint64_t* pay_off, uint64_t* len,
                              uint8_t* flags, uint32_t* mask, uint64_t* out_off, uint64_t* size, hipStream_t st);
// The reply rule over hvws_messages' piece table (msgs, mg_meta[2] pieces
// clamped to cap, per-segment seg_first / seg_count).  closed_in: device, nseg
// bytes or null; limit: nseg words; scratch: rep_scratch_words(cap) words, of
// which word `cap` receives the reply count; out / piece: cap entries.  by_rec:
// the table is hvws_messages_rfc's, "close is final" goes by the pieces' rec.
// fail (nseg words of hvws_check's fail_rec, or null; by_rec only): a piece
// whose rec is at or beyond its connection's word sends nothing, and a
// connection whose word is set gets RF_FAILED | RF_CLOSED.
uint64_t rep_scratch_words(uint64_t cap);
hipError_t launch_replies(const dmsg* msgs, const uint64_t* mg_meta, uint64_t cap, const uint64_t* seg_first,
                          const uint64_t* seg_count, uint32_t nseg, uint32_t policy, const uint8_t* closed_in,
                          uint64_t* limit, uint64_t* scratch, dtxmsg* out, uint64_t* piece, uint64_t* rep_first,
                          uint64_t* rep_count, uint8_t* flags, bool by_rec, hipStream_t st,
                          const uint64_t* fail = nullptr);
// hvws_fanout (hvws_fan.hip; include/hvws.h has the contract).  What its
// kernels read: the reply table of launch_replies (rep, piece, the count word
// clamped to rep_cap), the piece table it answers (pieces, mg_meta[2] clamped to
// piece_cap), dest_of / pub per segment (device; pub may be null), and the
// caller's subscription table.  rtopic (null: hvws_fanout): the topic per
// REPLY that launch_route left, in place of pub[segment] -- hvws_fanout_routed;
// rep is then the routed rows.
struct fan_tables {
    const dtxmsg* rep;
    const uint64_t* piece;
    const uint64_t* nrep_dev;
    uint64_t rep_cap;
    const dmsg* pieces;
    const uint64_t* mg_meta;
    uint64_t piece_cap;
    uint32_t nseg;
    const uint32_t* dest_of;
    const uint32_t* pub;
    const uint64_t* topic_first;
    const uint32_t* member;
    uint32_t ntopics;
    uint64_t nmember;
    uint32_t ndest;
    bool self;   // HVWS_FAN_SELF
    const uint32_t* rtopic = nullptr;
};
uint64_t fan_scratch_bytes(uint64_t cap);      // the edge scan over cap replies
uint32_t fan_sort_passes(uint32_t ndest);      // ceil(bits(2 ndest) / 8)
uint64_t fan_sort_groups(uint64_t nedges);     // workgroups of a sort pass
uint64_t fan_hist_words(uint64_t nedges);      // histogram, its scan and the scan's scratch
// The edge count: mark (nseg words), selfc (nseg words of 8 bytes) and segbad
// (nseg words) per segment, the scan in scratch (fan_scratch_bytes(rep_cap)),
// then meta[0..3] = edges before the self drop, deliveries, bad replies (their
// topic row leaves the member table, a member id is >= ndest, or their piece is
// none of the batch), replies.  No read leaves topic_first[0 .. ntopics] or
// member[0 .. nmember).  With rtopic the self edges and the row checks are per
// publication: selfc and segbad hold rep_cap words each, mark is not used.
hipError_t launch_fan_count(const fan_tables& in, uint32_t* mark, uint64_t* selfc, uint32_t* segbad, void* scratch,
                            uint64_t* meta, hipStream_t st);
// Expansion, sort and finish for nedges edges of which ndel are delivered (both
// read by the host from meta, bad == 0): key / val are the ping-pong pair
// arrays (nedges words each), hist fan_hist_words(nedges) words; out / reply:
// ndel entries, first / count: ndest.  *key_in: which of key[0], key[1] holds the
// sorted keys afterwards (its first ndel words are 2 * destination + (opcode == 8)
// of each delivery; hvws_budget.hip reads them).
hipError_t launch_fan_deliver(const fan_tables& in, const void* scratch, uint64_t nedges, uint64_t ndel, uint32_t* key[2],
                              uint32_t* val[2], uint64_t* hist, dtxmsg* out, uint64_t* reply, uint64_t* first,
                              uint64_t* count, int* key_in, hipStream_t st);
// The sort of launch_fan_deliver on its own: n pairs by the low 8 * passes bits
// of their keys, stable, between the ping-pong arrays; *cur says which of the
// two holds the pairs, before and after.  hist: fan_hist_words(n) words.
uint32_t fan_key_passes(uint64_t max_key);     // ceil(bits(max_key) / 8)
hipError_t launch_fan_sort(uint32_t* const key[2], uint32_t* const val[2], uint64_t n, uint32_t passes, uint64_t* hist,
                           int* cur, hipStream_t st);
// hvws_route (hvws_route.hip; include/hvws.h has the contract).  What its
// kernels read: the reply table and the piece table as fan_tables names them,
// dest_of per segment (device), and at most 12 bytes per TEXT / BINARY reply of
// the message call's output out[0, out_cap).
struct dsubev;   // mirrors hvws_sub_event (below)
enum : uint32_t { RK_OTHER = 0u, RK_PUB = 1u, RK_SUB = 2u, RK_UNSUB = 3u, RK_BAD = 4u, RK_STOPPED = 5u, RT_BAD = 1u };
struct route_tables {
    const dtxmsg* rep;
    const uint64_t* piece;
    const uint64_t* nrep_dev;
    uint64_t rep_cap;
    const dmsg* pieces;
    const uint64_t* mg_meta;
    uint64_t piece_cap;
    uint32_t nseg;
    const uint32_t* dest_of;
    uint32_t ntopics;
    const uint8_t* out;
    uint64_t out_cap;
};
// What they write: rows / topic / kind (rep_cap entries each), bad_reply and
// flags per segment, the dense event table ev (rep_cap entries), scratch
// (route_scratch_bytes(rep_cap)), meta (8 words): [0] events, [1..4] =
// publications, subscribes, unsubscribes, bad + stopped.
struct route_work {
    dtxmsg* rows;
    uint32_t* topic;
    uint8_t* kind;
    uint64_t* bad_reply;
    uint8_t* flags;
    dsubev* ev;
    void* scratch;
    uint64_t* meta;
};
uint64_t route_scratch_bytes(uint64_t cap);
// The scratch begins with the count scan's result, which stands until the next
// launch_route: four 32-bit words per reply, the {publications, subscribes,
// unsubscribes, bad + stopped} before it (hvws_retain.hip reads the event index
// of a SUB reply from words 1 and 2).
// The whole pass, no wait.  No read leaves [off, off + min(len, 12)) of a reply,
// nor out[0, out_cap).
hipError_t launch_route(const route_tables& t, const route_work& w, hipStream_t st);
// hvws_budget (hvws_budget.hip; include/hvws.h has the contract).  What its
// kernels read: the delivery table of launch_fan_deliver (rows, reply, n of them
// -- the host knows the count), its sorted keys, first / count per destination,
// and the caller's budgets (device, ndest words, or null: budget_all for all).
// F: bytes per fragment; maxlen: the longest message a row can name.
enum : uint32_t { BF_OVER = 1u };
struct budget_tables {
    const dtxmsg* rows;
    const uint64_t* reply;
    const uint32_t* key;
    uint64_t n;
    const uint64_t* first;
    const uint64_t* count;
    uint32_t ndest;
    const uint64_t* budget;
    uint64_t budget_all;
    uint64_t F, maxlen;
    bool masked;
};
// What they write: scratch (budget_scratch_words(n, ndest) words: the wire bytes
// before each delivery, their total, the scans' scratch), count2 / kept / flags
// per destination (kept: its kept wire bytes), first2 and byte_off (ndest + 1
// words each, the totals last), out / reply_out (n entries), meta (8 words):
// [0..3] = kept deliveries, kept bytes, dropped deliveries, destinations over.
struct budget_work {
    uint64_t* scratch;
    uint64_t* count2;
    uint64_t* kept;
    uint8_t* flags;
    uint64_t* first2;
    uint64_t* byte_off;
    dtxmsg* out;
    uint64_t* reply_out;
    uint64_t* meta;
};
uint64_t budget_scratch_words(uint64_t n, uint32_t ndest);
// The bytes the send emits for a message of len bytes (saturating): on the host,
// for the bound hvws_budget checks before it launches.
uint64_t budget_wire(uint64_t len, uint64_t F, int masked);
// The whole pass, no wait.  No read leaves budget[0 .. ndest).
hipError_t launch_budget(const budget_tables& t, const budget_work& w, hipStream_t st);
// hvws_subs_update (hvws_subs.hip; include/hvws.h has the contract).  dsubev
// mirrors hvws_sub_event.  What its kernels read: the caller's table, the
// events and dest_of (device copies; dest_of null: no implicit drops) and the
// reply call's per-segment flags.
struct dsubev {
    uint32_t op, topic, dest;
};
struct subs_tables {
    const uint64_t* topic_first;
    const uint32_t* member;
    uint32_t ntopics;
    uint64_t nmember;
    uint32_t ndest;
    const dsubev* ev;
    uint64_t nev;
    const uint32_t* dest_of;
    const uint8_t* rflags;
    uint32_t nseg;
    bool unique;   // HVWS_SUBS_UNIQUE
};
// Its work areas: drop (ndest words), the sort's pair arrays (nev words each)
// and hist (fan_hist_words(nev)), pk (nev words of 8 bytes), evfirst
// (ntopics + 1 words of 8 bytes: each topic's first sorted event), kind / eff / listed
// (nev bytes each), surv (nmember bytes), brow (nmember / 256 + 2 words: the
// row of every 256th listing), erank (subs_event_rank_words(nev)),
// lrank (subs_rank_words(nmember)), meta (10 words of 8 bytes).
struct subs_work {
    uint32_t* drop;
    uint32_t* key[2];
    uint32_t* val[2];
    uint64_t* hist;
    uint64_t* pk;
    uint64_t* evfirst;
    uint8_t* kind;
    uint8_t* eff;
    uint8_t* listed;
    uint8_t* surv;
    uint32_t* brow;
    uint64_t* erank;
    uint64_t* lrank;
    uint64_t* meta;
};
uint64_t subs_rank_words(uint64_t n);
uint64_t subs_event_rank_words(uint64_t nev);
// Everything up to the counts: meta[0..5] = new nmember, listings kept, added,
// removed, destinations dropped as closed, bad (the table is not dense or holds
// a member id >= ndest).  No read leaves topic_first[0 .. ntopics],
// member[0 .. nmember) or rflags[0 .. nseg); neither output is touched.
hipError_t launch_subs_count(const subs_tables& t, const subs_work& w, hipStream_t st);
// The placement, for a table launch_subs_count found good: first_out
// (ntopics + 1 words) and member_out[0 .. newn).
hipError_t launch_subs_place(const subs_tables& t, const subs_work& w, uint64_t newn, uint64_t* first_out,
                             uint32_t* member_out, hipStream_t st);
// The merge of hvws_subs_update_routed.  What its kernels read: the route
// pass's event table (rt_ev, its count word clamped to rt_cap), per segment the
// reply call's flags, the route pass's flags and its device copy of dest_of,
// the budget pass's flags per destination (nover of them; 0: none are read)
// and the uploaded host events.
struct subs_merge {
    const dsubev* rt_ev;
    const uint64_t* rt_nev;
    uint64_t rt_cap;
    const uint8_t* rflags;
    const uint8_t* rtflags;
    const uint32_t* dest_of;
    uint32_t nseg;
    const uint8_t* bflags;
    uint32_t nover;
    const dsubev* host_ev;
    uint64_t nev;
};
uint64_t subs_merge_words(uint32_t nseg, uint32_t nover);
// Two scans (scratch: subs_merge_words words) and the append, no wait: out
// (rt_cap + nseg + nover + nev entries) = the route's events, a DROP per closed
// or malformed segment, a DROP per OVER destination, the host's events;
// meta[0..4] = those four counts and their sum.
hipError_t launch_subs_merge(const subs_merge& t, uint64_t* scratch, dsubev* out, uint64_t* meta, hipStream_t st);
// hvws_retain (hvws_retain.hip; include/hvws.h has the contract).  dretained
// mirrors hvws_retained.  What its kernels read: the routed rows, topic and
// kind per reply, the event table and the count scan's result that
// launch_route left (rt_ex: route_scratch_bytes' note), the reply count word
// clamped to rep_cap, the reply call's first / count per segment, the winning
// bodies in the message call's output out[0, out_cap), and the caller's entry
// ret[t] of a topic subscribed to and not published to this turn.  They write
// ret[t] of every topic published to and store[t * slot, t * slot + len) of
// every topic stored.
struct dretained {
    uint64_t len;
    uint32_t flags, set;
};
constexpr uint64_t RETAIN_TILE = 4096;   // store bytes one workgroup of the copy covers per step
constexpr uint64_t RETAIN_GRID = 2048;   // its largest grid: 8 workgroups per CU of a 256-CU device
struct retain_tables {
    const dtxmsg* rows;
    const uint32_t* topic;
    const uint8_t* kind;
    const uint32_t* rt_ex;
    const dsubev* ev;
    const uint64_t* nrep_dev;
    uint64_t rep_cap;
    const uint64_t* rep_first;
    const uint64_t* rep_count;
    uint32_t nseg;
    uint32_t ntopics;
    const uint8_t* out;
    uint64_t out_cap;
    uint8_t* store;
    uint64_t slot;
    dretained* ret;
};
// What they write besides: win (ntopics words), scratch
// (retain_scratch_bytes(rep_cap)), the copy plan pl_* (min(rep_cap, ntopics) + 1
// entries each: first tile, source offset, store offset, length of every stored
// winner, dense, in reply order), the snapshot rows with topic and reply
// (rep_cap entries each), first / count per segment, meta (8 words): [0]
// snapshot rows, [1..5] = stored, cleared empty, cleared oversize, bytes
// copied, snapshot rows.
struct retain_work {
    uint32_t* win;
    void* scratch;
    uint64_t* pl_tile;
    uint64_t* pl_src;
    uint64_t* pl_dst;
    uint64_t* pl_len;
    dtxmsg* rows;
    uint32_t* topic;
    uint64_t* reply;
    uint64_t* first;
    uint64_t* count;
    uint64_t* meta;
};
uint64_t retain_scratch_bytes(uint64_t cap);
// The whole pass, no wait.  No read leaves [off & ~15, off + len rounded up to
// 16) of a winning row, nor out[0, out_cap); nothing reads the store.
hipError_t launch_retain(const retain_tables& t, const retain_work& w, hipStream_t st);
// hvws_envelope (hvws_envelope.hip; include/hvws.h has the contract).  What its
// kernels read: the routed rows, topic and kind per reply that launch_route
// left, the reply count word clamped to rep_cap, with `sender` the piece each
// reply answers, the piece table and dest_of per segment (device), and the
// bodies in the message call's output out[0, out_cap).  They write env[0,
// env_cap): reply i's bytes at its offset e_i, nothing between replies.
constexpr uint64_t ENV_TILE = 1024;   // bytes of env one workgroup of the copy (one wave) covers per step
constexpr uint64_t ENV_GRID = 8192;   // its largest grid: 32 waves per CU of a 256-CU device
struct env_tables {
    const dtxmsg* rows;
    const uint32_t* topic;
    const uint8_t* kind;
    const uint64_t* piece;
    const uint64_t* nrep_dev;
    uint64_t rep_cap;
    const dmsg* pieces;
    const uint64_t* mg_meta;
    uint64_t piece_cap;
    uint32_t nseg;
    const uint32_t* dest_of;
    const uint8_t* out;
    uint64_t out_cap;
    uint8_t* env;
    uint64_t env_cap;
    bool sender;   // HVWS_ENV_SENDER
    // hvws_envelope_sequenced: the number per reply that launch_sequence left
    // (rep_cap entries); a publication's line then ends ` #<seq>`.  Null:
    // hvws_envelope.  The host picks the kernels by it; no kernel tests it.
    const uint64_t* seq = nullptr;
};
// What they write besides: scratch (env_scratch_bytes(rep_cap)), the enveloped
// rows (rep_cap entries; rrows: the same with length 0 where a publication's
// body is empty, the rows launch_retain takes), the copy plan pl_* (rep_cap + 1 entries each: first
// tile, source offset, offset in env and length of every body copied, dense, in
// reply order), meta (8 words): [0..3] = enveloped publications, replies copied
// verbatim, bytes written, bytes of env spanned.
struct env_work {
    void* scratch;
    dtxmsg* rows;
    dtxmsg* rrows;
    uint64_t* pl_tile;
    uint64_t* pl_src;
    uint64_t* pl_dst;
    uint64_t* pl_len;
    uint64_t* meta;
};
uint64_t env_scratch_bytes(uint64_t cap);
// The whole pass, no wait.  No read leaves [off & ~15, off + len rounded up to
// 16) of a copied row, nor out[0, out_cap); no write leaves reply i's [e_i, e_i +
// bytes), nor env[0, env_cap).
hipError_t launch_envelope(const env_tables& t, const env_work& w, hipStream_t st);
// hvws_sequence (hvws_seq.hip; include/hvws.h has the contract).  What its
// kernels read: topic and kind per reply that launch_route left, the reply
// count word clamped to rep_cap, and the caller's counter d_seq[t] of every
// topic published to this turn.  They write d_seq[t] of those topics alone.
struct seq_tables {
    const uint32_t* topic;
    const uint8_t* kind;
    const uint64_t* nrep_dev;
    uint64_t rep_cap;
    uint32_t ntopics;
    uint64_t* d_seq;
};
// What they write besides: the sort's pair arrays (rep_cap words each) and hist
// (fan_hist_words(rep_cap)), scratch (seq_scratch_bytes(rep_cap)), seq (rep_cap
// entries: the number of a publication, 0 for every other slot), meta (8
// words): [0..1] = publications numbered, distinct topics published to.
struct seq_work {
    uint32_t* key[2];
    uint32_t* val[2];
    uint64_t* hist;
    void* scratch;
    uint64_t* seq;
    uint64_t* meta;
};
uint64_t seq_scratch_bytes(uint64_t cap);
// The whole pass, no wait.  No read or write leaves d_seq[0 .. ntopics); the
// counters are stored by a kernel of their own behind the one that reads them.
hipError_t launch_sequence(const seq_tables& t, const seq_work& w, hipStream_t st);
// hvws_check (hvws_check.hip; include/hvws.h has the rule).  Reads the frame
// table's info / length (nfr_dev, cap as for launch_utf8), bases, the piece
// table of hvws_messages_rfc (mg_meta[2] pieces clamped to pcap), at most 125
// bytes per Close piece of that call's output out[0, out_len), and u8_bad (the
// bad[] of hvws_utf8; read only with CK_TEXT_UTF8).  scratch:
// check_scratch_bytes(cap); viol: cap + pcap bytes; state_in (device, nullptr:
// all fresh) -> state_out, fail, why, code (nseg entries each).
enum : uint32_t {
    CK_HEADER = 1u, CK_SEQUENCE = 2u, CK_CLOSE_BODY = 4u, CK_CLOSE_UTF8 = 8u, CK_TEXT_UTF8 = 16u, CK_SIZE = 32u,
    CK_ALL = 63u,
    CK_OPEN = 1u, CK_FAILED = 2u   // the state word
};
uint64_t check_scratch_bytes(uint64_t cap);
hipError_t launch_check(const uint32_t* info, const uint64_t* length, const uint64_t* nfr_dev, uint64_t cap,
                        const uint64_t* bases, uint32_t nseg, const dmsg* msgs, const uint64_t* mg_meta, uint64_t pcap,
                        const uint8_t* out, uint64_t out_len, const uint64_t* u8_bad, uint32_t classes,
                        uint64_t max_message, const uint32_t* state_in, void* scratch, uint8_t* viol, uint32_t* state_out,
                        uint64_t* fail, uint32_t* why, uint16_t* code, hipStream_t st);
// Predicted frames above which a uniform segment is verified grid-wide (k_verify).
uint64_t spec_min();
uint64_t set_spec_min(uint64_t v);   // 0 = default; returns the previous value
// k_unmask geometry variants (threads x chunks/thread, XCD-ordered tiles)
int unmask_variant();                      // the forced geometry, else the large-batch default
int unmask_variant_for(uint64_t rx_len);   // the geometry a batch of rx_len bytes runs with
int set_unmask_variant(int v);             // -1 = by batch size; -2 if out of range
int unmask_variant_count();
uint64_t unmask_tile(int variant);         // bytes per workgroup tile
const char* unmask_name(int variant);
hipError_t launch_unmask(int variant, uint8_t* rx, uint64_t rx_len, dframes fr, const uint32_t* tile_first,
                         const uint32_t* tile_key, const uint8_t* tile_kind, const uint64_t* nfr_dev, hipStream_t st,
                         uint32_t pieces = 1, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
hipError_t launch_tile_class(const uint64_t* off, const uint64_t* len, const uint32_t* keyrot, const uint64_t* nfr_dev,
                             const uint32_t* tile_first, uint32_t* tile_key, uint8_t* tile_kind, uint64_t ntiles,
                             uint64_t tile, uint64_t rx_len, hipStream_t st);
// Tile index + tile classes for k_unmask in one sequence (fill, scatter,
// fused fixup/classify); tile_first must hold ntiles + 8 entries.
hipError_t launch_unmask_tiles(const uint64_t* off, const uint64_t* len, const uint32_t* keyrot, const uint64_t* nfr_dev,
                               uint32_t* tile_first, uint32_t* tile_key, uint8_t* tile_kind, uint64_t ntiles,
                               uint64_t tile, uint64_t rx_len, hipStream_t st);
hipError_t launch_stream_xor(int variant, uint8_t* d, uint64_t n, uint32_t pattern, hipStream_t st);
hipError_t launch_xor_span(uint8_t* d, uint64_t n, uint32_t key, uint32_t phase, hipStream_t st);
hipError_t launch_noop(hipStream_t st);   // see hvws_dev_free

// Synthetic data (hvws_synth.hip).
hipError_t launch_synth(uint8_t* buf, uint64_t buf_len, uint64_t seed, uint64_t nframes,
                        const uint64_t* frame_off, const uint8_t* flags, const uint32_t* mask,
                        const uint64_t* length, const uint8_t* text, const uint64_t* frame_size,
                        const uint32_t* tile_first, int mode, unsigned long long* mismatches,
                        hipStream_t st);
hipError_t launch_digest(const uint8_t* buf, uint64_t len, unsigned long long* out, hipStream_t st);
hipError_t launch_frame_sizes(const uint8_t* flags, const uint64_t* length, uint64_t nframes,
                              uint64_t* out, hipStream_t st);
uint64_t synth_tile();

// Transmit side (hvws_tx.hip).
// out[i] = sum(in[0..i)), *total = sum(in); tmp >= 4 * ceil(n / 1024) + 64 words.
hipError_t launch_exclusive_scan(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* tmp, uint64_t* total,
                                 hipStream_t st);
// stat[1] += frames whose payload range leaves [0, plen) or that are masked
// without a key table; stat[2] += frames breaking the uniform layout (size
// or length other than frame 0's, payload offset step other than frame 1's or
// negative); stat[3..5] = pay_off[0], pay_off[1] - pay_off[0], len[0].
hipError_t launch_tx_check(const uint64_t* pay_off, const uint64_t* len, const uint8_t* flags, const uint32_t* mask,
                           const uint64_t* size, uint64_t n, uint64_t plen, uint64_t* stat, hipStream_t st);
// k_build geometry for a batch of out_len output bytes in n frames
// ($HVWS_EXPERIMENT build, else by the mean frame size), its tile and its name
int tx_variant(uint64_t out_len, uint64_t n);
uint64_t tx_tile(int v);   // output bytes per k_build workgroup
const char* build_kernel_name(int v);
// The transmit tile index and (span != nullptr: 2 words per k_build tile)
// source spans in three launches: one fill of both, one pass over the frames
// doing the tile scatter and the span runs together, k_tile_fixup (in place
// of a tile index's fill, scatter and fixup plus a span fill and pass).
hipError_t launch_tx_index(const uint64_t* out_off, const uint64_t* size, const uint64_t* pay_off, const uint64_t* len,
                           const uint8_t* flags, uint64_t n, uint64_t ntiles, uint64_t tile, uint32_t* tile_first,
                           uint64_t* span, hipStream_t st);
// span: from launch_tx_index, or nullptr (boundary tiles load their records
// first).  uni (host array {stride, header bytes, pay_off[0], payload offset
// step}, stride != 0): a uniform layout -- every tile finds its frame range and
// span from its position, tile_first and span are not read (no index pass).
hipError_t launch_build(uint8_t* out, uint64_t out_len, const uint8_t* pay, uint64_t plen, const uint64_t* pay_off,
                        const uint64_t* len, const uint8_t* flags, const uint32_t* mask, const uint64_t* out_off,
                        const uint64_t* size, const uint32_t* tile_first, const uint64_t* span, uint64_t n, int v,
                        hipStream_t st, const uint64_t* uni = nullptr);

}  // namespace hvws
