// hvws_fan.hip -- the table kernels of hvws_fanout (include/hvws.h has the
// contract): the reply table of hvws_replies expanded through a subscription
// table and ordered by destination connection, the job of the reference's
// TcpServerTmpl::broadcast / foreachChannel (evpp/TcpServer.h) for a whole
// batch.  No pass over the payload: the send reads each message's bytes where
// the message call left them, once per delivery.
//
//   the edge count   per segment with a publication among its replies, one
//                    workgroup walks the segment's topic row once: how often the
//                    segment's own destination is listed (the self edges) and
//                    whether a member id lies outside [0, ndest).  Then one
//                    device-wide scan over the replies (the scan of hvws_dev.h)
//                    carries {edges, deliveries, bad}: edges before the self drop
//                    (what the expansion and the sort run over), deliveries after
//                    it (what the host waits for), all saturating.  In the
//                    routed form (hvws_fanout_routed: a topic per reply from
//                    hvws_route) each publication may reach another row, so the
//                    walk is per publishing reply, one wavefront each: its work
//                    is the edge count, the order of the expansion's.
//   the expansion    one thread per EDGE: edge e finds its reply by binary search
//                    over the scan and writes the pair (key, reply), key =
//                    2 * destination + (opcode == 8).  A dropped self edge gets
//                    the key 2 * ndest: it sorts behind every delivery and is cut
//                    off there.  One publication to 100 000 members spreads over
//                    the grid as evenly as 100 000 publications to one.
//   the sort         LSD radix sort of the pairs by key, 8 bits per pass,
//                    ceil(bits(2 * ndest) / 8) passes, stable: the edges are
//                    produced in (reply, listing) order, so the sort by key alone
//                    gives the contract's order.  Per pass a digit histogram per
//                    workgroup (LDS atomics: they count, they never place), one
//                    device scan of the 256 x workgroups counts, and a scatter
//                    that ranks equal digits inside the workgroup in thread order:
//                    eight wave ballots give a lane its peers, an LDS table of 4
//                    waves x 256 digits the waves before it.  The output is the
//                    same on every run.
//   the finish       delivery k gathers its hvws_tx_msg from the reply table;
//                    destination d finds its range by two binary searches over
//                    the sorted keys (no destination depends on another's run).
//
// Traffic per edge: 24 B of scan state searched (log2 replies reads, cached),
// 8 B written by the expansion; per sort pass 4 B read by the histogram, 8 B
// read and 8 B written by the scatter, and 256 counters of 8 B per 2048 pairs
// written, scanned and read; 4 B and a reply row read, 32 B written by the finish.
#include "hvws_dev.h"

namespace hvws {

namespace {

struct fan3 {
    uint64_t edges, del, bad;
};
__device__ __forceinline__ uint64_t fan_sat(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
__device__ __forceinline__ fan3 scan_op(const fan3& a, const fan3& b) {
    return fan3{fan_sat(a.edges, b.edges), fan_sat(a.del, b.del), fan_sat(a.bad, b.bad)};
}

constexpr uint32_t FAN_NONE = 0xFFFFFFFFu;
constexpr uint32_t FAN_T = 256;               // threads per sort workgroup: 4 waves
constexpr uint32_t FAN_ITEMS = 8;             // pairs per thread (4 and 16 measured beside it)
constexpr uint32_t FAN_TILE = FAN_T * FAN_ITEMS;

// Over fan_tables (hvws_internal.h).  fan_seg(t, i): the segment of the piece
// reply i answers (nseg for a piece outside the batch: counted as bad).
__device__ __forceinline__ uint64_t fan_replies(const fan_tables& t) {
    const uint64_t d = *t.nrep_dev;
    return d < t.rep_cap ? d : t.rep_cap;
}
__device__ __forceinline__ uint32_t fan_seg(const fan_tables& t, uint64_t i) {
    const uint64_t p = t.piece[i];
    const uint64_t np = t.mg_meta[2] < t.piece_cap ? t.mg_meta[2] : t.piece_cap;
    if (p >= np) return t.nseg;
    const uint32_t s = t.pieces[p].seg;
    return s < t.nseg ? s : t.nseg;
}
__device__ __forceinline__ uint32_t fan_topic(const fan_tables& t, uint32_t s) {
    if (!t.pub) return FAN_NONE;
    const uint32_t tp = t.pub[s];
    return tp < t.ntopics ? tp : FAN_NONE;   // the host refused any other value but NONE
}
// The topic of reply i of segment s, and where its self count and bad mark
// stand: per segment, or per reply in the routed form (hvws_fanout_routed),
// where a reply's topic is hvws_route's.
__device__ __forceinline__ uint32_t fan_topic_of(const fan_tables& t, uint64_t i, uint32_t s) {
    if (!t.rtopic) return fan_topic(t, s);
    const uint32_t tp = t.rtopic[i];
    return tp < t.ntopics ? tp : FAN_NONE;
}
__device__ __forceinline__ uint64_t fan_slot(const fan_tables& t, uint64_t i, uint32_t s) { return t.rtopic ? i : s; }
// topic tp's row, true when it lies inside the member table
__device__ __forceinline__ bool fan_row(const fan_tables& t, uint32_t tp, uint64_t& a, uint64_t& b) {
    a = t.topic_first[tp];
    b = t.topic_first[tp + 1];
    return a <= b && b <= t.nmember;
}

__device__ __forceinline__ bool is_pub(uint32_t flags) {
    const uint32_t op = flags & F_OPMASK;
    return op == 1 || op == 2;
}

// mark[s] = 1 for a segment with a publication among its replies (zero on entry)
__global__ __launch_bounds__(256) void k_fan_mark(fan_tables in, uint32_t* __restrict__ mark) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= fan_replies(in)) return;
    if (!is_pub(in.rep[i].flags)) return;
    const uint32_t s = fan_seg(in, i);
    if (s < in.nseg && fan_topic(in, s) != FAN_NONE) mark[s] = 1u;
}

// One workgroup per segment: selfc[s] = listings of dest_of[s] in the segment's
// topic row, segbad[s] = 1 for a row outside the member table or a member id
// outside [0, ndest).  Unmarked segments read nothing and get zeros.
__global__ __launch_bounds__(256) void k_fan_self(fan_tables in, const uint32_t* __restrict__ mark,
                                                  uint64_t* __restrict__ selfc, uint32_t* __restrict__ segbad) {
    __shared__ unsigned long long s_self;
    __shared__ uint32_t s_bad;
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        s_self = 0;
        s_bad = 0;
    }
    __syncthreads();
    if (mark[s]) {   // uniform over the workgroup
        const uint32_t tp = fan_topic(in, s);
        uint64_t a, b;
        if (!fan_row(in, tp, a, b)) {
            if (t == 0) s_bad = 1u;
        } else {
            const uint32_t me = in.dest_of[s];
            uint64_t n = 0;
            uint32_t bad = 0;
            for (uint64_t k = a + t; k < b; k += blockDim.x) {
                const uint32_t d = in.member[k];
                n += d == me ? 1u : 0u;
                bad |= d >= in.ndest ? 1u : 0u;
            }
            const uint64_t mb = __ballot(bad != 0);
#pragma unroll
            for (int o = 32; o; o >>= 1) n += __shfl_down(n, o);
            if ((t & 63u) == 0) {
                if (n) atomicAdd(&s_self, (unsigned long long)n);
                if (mb) atomicOr(&s_bad, 1u);
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        selfc[s] = s_self;
        segbad[s] = s_bad;
    }
}

// The routed form: one wavefront per publishing reply walks that reply's topic
// row once: selfc[i] = listings of the sender's own destination, repbad[i] = 1
// for a row outside the member table or a member id outside [0, ndest).  The
// work is the edge count, as the expansion's.  Other replies read and write
// nothing: fan_load does not look at their words.
__global__ __launch_bounds__(256) void k_fan_self_reply(fan_tables in, uint64_t* __restrict__ selfc,
                                                        uint32_t* __restrict__ repbad) {
    const uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / 64u) + (threadIdx.x >> 6);   // uniform over the wave
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= fan_replies(in)) return;
    if (!is_pub(in.rep[i].flags)) return;
    const uint32_t s = fan_seg(in, i);
    if (s >= in.nseg) return;
    const uint32_t tp = fan_topic_of(in, i, s);
    if (tp == FAN_NONE) return;
    uint64_t a, b, n = 0;
    uint32_t bad = 0;
    if (!fan_row(in, tp, a, b)) {
        bad = 1u;
    } else {
        const uint32_t me = in.dest_of[s];
        for (uint64_t k = a + lane; k < b; k += 64) {
            const uint32_t d = in.member[k];
            n += d == me ? 1u : 0u;
            bad |= d >= in.ndest ? 1u : 0u;
        }
    }
    const uint64_t mb = __ballot(bad != 0);
#pragma unroll
    for (int o = 32; o; o >>= 1) n += __shfl_down(n, o);
    if (lane == 0) {
        selfc[i] = n;
        repbad[i] = mb ? 1u : 0u;
    }
}

// What reply i adds to the scan.  Replies at or beyond the count add the identity.
struct fan_load {
    fan_tables in;
    const uint64_t* selfc;
    const uint32_t* segbad;
    __device__ __forceinline__ fan3 operator()(uint64_t i) const {
        if (i >= fan_replies(in)) return fan3{};
        const uint32_t s = fan_seg(in, i);
        if (s >= in.nseg) return fan3{0, 0, 1};
        if (!is_pub(in.rep[i].flags)) return fan3{1, 1, 0};   // PONG, CLOSE: to the sender alone
        const uint32_t tp = fan_topic_of(in, i, s);
        if (tp == FAN_NONE) return fan3{};
        const uint64_t x = fan_slot(in, i, s);
        if (segbad[x]) return fan3{0, 0, 1};
        uint64_t a, b;
        fan_row(in, tp, a, b);
        const uint64_t e = b - a, own = in.self ? 0 : selfc[x];
        return fan3{e, e - own, 0};
    }
};

// meta[0..3] = edges, deliveries, bad replies, replies
__global__ void k_fan_meta(fan_tables in, const fan3* __restrict__ total, uint64_t* __restrict__ meta) {
    const fan3 t = *total;
    meta[0] = t.edges;
    meta[1] = t.del;
    meta[2] = t.bad;
    meta[3] = fan_replies(in);
}

// One thread per edge: the pair the sort takes.
__global__ __launch_bounds__(256) void k_fan_expand(fan_tables in, const fan3* __restrict__ ex, uint64_t nedges,
                                                    uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t cnt = fan_replies(in);
    if (e >= nedges || cnt == 0) return;
    // the last reply whose first edge is <= e: replies without edges share
    // their successor's first edge and are passed over
    uint64_t lo = 0, hi = cnt;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ex[mid].edges <= e) lo = mid;
        else hi = mid;
    }
    const uint64_t j = e - ex[lo].edges;
    const uint32_t fl = in.rep[lo].flags;
    const uint32_t s = fan_seg(in, lo);   // < nseg: the host saw no bad reply
    const uint32_t me = in.dest_of[s];
    uint32_t k;
    if (is_pub(fl)) {
        uint64_t a, b;
        fan_row(in, fan_topic_of(in, lo, s), a, b);
        const uint64_t at = a + j < in.nmember ? a + j : in.nmember - 1;   // a + j < b <= nmember
        const uint32_t d = in.member[at];
        k = d == me && !in.self ? 2u * in.ndest : 2u * d;
    } else {
        k = 2u * me + ((fl & F_OPMASK) == 8 ? 1u : 0u);
    }
    key[e] = k;
    val[e] = (uint32_t)lo;
}

// ------------------------------------------------------------------ the sort

// Pair i of a workgroup's tile sits at tile + item * FAN_T + thread: the tile's
// order is item by item, and within an item thread by thread.

// hist[digit * nwg + workgroup] = the tile's pairs with that digit
__global__ __launch_bounds__(FAN_T) void k_fan_hist(const uint32_t* __restrict__ key, uint64_t n, uint32_t shift,
                                                    uint64_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    const uint32_t t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const uint64_t tile = (uint64_t)blockIdx.x * FAN_TILE;
#pragma unroll
    for (uint32_t it = 0; it < FAN_ITEMS; ++it) {
        const uint64_t i = tile + it * FAN_T + t;
        if (i < n) atomicAdd(&h[(key[i] >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    hist[(uint64_t)t * gridDim.x + blockIdx.x] = h[t];
}

// base: the exclusive scan of hist.  Every pair's place is its digit's base for
// this workgroup, plus the pairs with that digit in the tile's earlier items,
// in the item's earlier waves, and in the wave's lower lanes.
__global__ __launch_bounds__(FAN_T) void k_fan_scatter(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                       uint64_t n, uint32_t shift, const uint64_t* __restrict__ base,
                                                       uint32_t* __restrict__ key_out, uint32_t* __restrict__ val_out) {
    __shared__ uint64_t run[256];          // the next place of each digit
    __shared__ uint32_t wcnt[FAN_T / 64][256];   // this item's pairs per wave and digit
    const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
    run[t] = base[(uint64_t)t * gridDim.x + blockIdx.x];
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) wcnt[v][t] = 0;
    __syncthreads();
    const uint64_t tile = (uint64_t)blockIdx.x * FAN_TILE;
    const uint64_t below = lane ? ~0ull >> (64u - lane) : 0ull;
    for (uint32_t it = 0; it < FAN_ITEMS; ++it) {
        const uint64_t i = tile + it * FAN_T + t;
        const bool on = i < n;
        const uint32_t k = on ? key[i] : 0u, v = on ? val[i] : 0u;
        const uint32_t d = (k >> shift) & 0xFFu;
        // the lanes of this wave that hold the same digit
        uint64_t peers = __ballot(on);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const uint64_t m = __ballot((d >> b) & 1u);
            peers &= (d >> b) & 1u ? m : ~m;
        }
        const uint32_t before = (uint32_t)__popcll(peers & below);
        if (on && before == 0) wcnt[w][d] = (uint32_t)__popcll(peers);   // the lowest peer writes
        __syncthreads();
        if (on) {
            uint64_t at = run[d] + before;
            for (uint32_t u = 0; u < w; ++u) at += wcnt[u][d];
            key_out[at] = k;
            val_out[at] = v;
        }
        __syncthreads();
        run[t] += (uint64_t)wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) wcnt[u][t] = 0;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- the finish

__global__ __launch_bounds__(256) void k_fan_rows(const uint32_t* __restrict__ val, uint64_t ndel,
                                                  const dtxmsg* __restrict__ rep, dtxmsg* __restrict__ out,
                                                  uint64_t* __restrict__ reply) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ndel) return;
    const uint32_t i = val[k];
    out[k] = rep[i];
    reply[k] = i;
}

// the first of key[0 .. n) that is >= x
__device__ __forceinline__ uint64_t fan_lower(const uint32_t* key, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (key[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_fan_dests(const uint32_t* __restrict__ key, uint64_t ndel, uint32_t ndest,
                                                   uint64_t* __restrict__ first, uint64_t* __restrict__ count) {
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= ndest) return;
    const uint64_t a = fan_lower(key, ndel, 2 * d), b = fan_lower(key, ndel, 2 * d + 2);
    first[d] = a;
    count[d] = b - a;
}

}  // namespace

uint64_t fan_scratch_bytes(uint64_t cap) { return (cap + 16 + scan_tmp_words(cap)) * sizeof(fan3); }
uint32_t fan_key_passes(uint64_t max_key) {
    uint32_t bits = 0;
    for (uint64_t v = max_key; v; v >>= 1) ++bits;
    return (bits + 7) / 8;
}
uint32_t fan_sort_passes(uint32_t ndest) { return fan_key_passes(2ull * ndest); }
uint64_t fan_sort_groups(uint64_t nedges) { return (nedges + FAN_TILE - 1) / FAN_TILE; }
uint64_t fan_hist_words(uint64_t nedges) {
    const uint64_t h = 256 * fan_sort_groups(nedges);
    return 2 * h + 16 + scan_tmp_words(h);
}

hipError_t launch_fan_count(const fan_tables& in, uint32_t* mark, uint64_t* selfc, uint32_t* segbad, void* scratch,
                            uint64_t* meta, hipStream_t st) {
    fan3* ex = reinterpret_cast<fan3*>(scratch);
    fan3* total = ex + in.rep_cap;   // one value; 16 are set aside
    fan3* tmp = ex + in.rep_cap + 16;
    const uint32_t rb = (uint32_t)((in.rep_cap + 255) / 256);
    if (in.rtopic) {   // per publication: four replies per workgroup
        if (in.rep_cap) hipLaunchKernelGGL(k_fan_self_reply, dim3((uint32_t)((in.rep_cap + 3) / 4)), dim3(256), 0, st, in, selfc, segbad);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    } else if (in.nseg) {
        hipError_t e = hipMemsetAsync(mark, 0, (uint64_t)in.nseg * 4, st);
        if (e != hipSuccess) return e;
        if (rb) hipLaunchKernelGGL(k_fan_mark, dim3(rb), dim3(256), 0, st, in, mark);
        hipLaunchKernelGGL(k_fan_self, dim3(in.nseg), dim3(256), 0, st, in, mark, selfc, segbad);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const fan_load load{in, selfc, segbad};
    hipError_t e = launch_scan_of(load, ex, in.rep_cap, tmp, total, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fan_meta, dim3(1), dim3(1), 0, st, in, total, meta);
    return hipGetLastError();
}

hipError_t launch_fan_sort(uint32_t* const key[2], uint32_t* const val[2], uint64_t n, uint32_t passes, uint64_t* hist,
                           int* cur, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uint64_t nwg = fan_sort_groups(n), h = 256 * nwg;
    uint64_t* base = hist + h;
    uint64_t* total = base + h;   // one value; 16 are set aside
    uint64_t* tmp = total + 16;
    int c = *cur;
    for (uint32_t p = 0; p < passes; ++p, c ^= 1) {
        hipLaunchKernelGGL(k_fan_hist, dim3((uint32_t)nwg), dim3(FAN_T), 0, st, key[c], n, 8 * p, hist);
        const hipError_t e = launch_scan_of(scan_from_array<uint64_t>{hist}, base, h, tmp, total, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_fan_scatter, dim3((uint32_t)nwg), dim3(FAN_T), 0, st, key[c], val[c], n, 8 * p, base,
                           key[c ^ 1], val[c ^ 1]);
    }
    *cur = c;
    return hipGetLastError();
}

hipError_t launch_fan_deliver(const fan_tables& in, const void* scratch, uint64_t nedges, uint64_t ndel, uint32_t* key[2],
                              uint32_t* val[2], uint64_t* hist, dtxmsg* out, uint64_t* reply, uint64_t* first,
                              uint64_t* count, int* key_in, hipStream_t st) {
    int cur = 0;
    if (nedges) {
        hipLaunchKernelGGL(k_fan_expand, dim3((uint32_t)((nedges + 255) / 256)), dim3(256), 0, st, in,
                           reinterpret_cast<const fan3*>(scratch), nedges, key[0], val[0]);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_fan_sort(key, val, nedges, fan_sort_passes(in.ndest), hist, &cur, st);
        if (e != hipSuccess) return e;
        if (ndel)
            hipLaunchKernelGGL(k_fan_rows, dim3((uint32_t)((ndel + 255) / 256)), dim3(256), 0, st, val[cur], ndel, in.rep,
                               out, reply);
    }
    hipLaunchKernelGGL(k_fan_dests, dim3((in.ndest + 255) / 256), dim3(256), 0, st, key[cur], ndel, in.ndest, first, count);
    *key_in = cur;
    return hipGetLastError();
}

}  // namespace hvws
