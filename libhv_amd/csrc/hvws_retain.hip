// hvws_retain.hip -- the kernels of hvws_retain (include/hvws.h has the
// contract): each topic's last publication of the turn kept in the caller's
// device-resident store, and a snapshot row for every subscribe of the turn
// whose topic holds a message afterwards.  The reference has no counterpart:
// its onmessage is user code.  Runs over what hvws_route left: the routed rows,
// topic and kind per reply, the event table.
//
//   the pick     one thread per reply: a publication takes atomicMax of
//                (reply index + 1) on its topic's word (zero on entry): a
//                maximum, so the order the threads run in does not show.
//   the plan     one device-wide scan over the replies (the scan of
//                hvws_dev.h) of {copy tiles, bytes, snapshot rows, stored,
//                cleared empty, cleared oversize}: a reply counts as a winner
//                where its topic's word names it, a subscribe counts where its
//                topic is retained after the update -- by this turn's winner if
//                there is one, by the caller's entry otherwise.  The total is
//                the pass's totals; the value before reply i says where i's
//                plan entry and snapshot row go.  No atomic places either.
//   the finish   one thread per reply: a winner writes its topic's entry and,
//                where it stores, its entry of the dense copy plan; a subscribe
//                of a retained topic writes its snapshot row, topic and reply;
//                one thread per segment: the segment's range of rows, from the
//                reply call's first / count and the scan.
//   the copy     the payload path.  Work is cut by destination tile of
//                RETAIN_TILE bytes, not by message: the grid's workgroups take
//                equal runs of consecutive tiles, each finds its first winner
//                by binary search over the plan's tile offsets and walks on
//                from there.  Per 16-byte chunk of a slot (slots are 16-byte
//                aligned) two aligned 16-byte loads of the source and a funnel
//                shift -- one load where the phases agree -- then one 16-byte
//                store, or byte stores for the body's last partial chunk.
//
// Traffic per reply: 24 B row + 4 B topic + 1 B kind read by the pick and again
// by the plan and the finish, 32 B of scan state written and read; per winner
// 16 B entry and 32 B plan; per snapshot row 24 + 4 + 8 B.  Per body byte: one
// read (plus at most 31 B around the body) and one write.
#include "hvws_dev.h"

namespace hvws {

namespace {

constexpr uint32_t RETAIN_T = 256;   // threads per workgroup of the copy: one 16-byte chunk each per tile
static_assert(RETAIN_TILE == RETAIN_T * 16, "a tile is one chunk per thread");

struct ret6 {
    uint64_t tiles, bytes;
    uint32_t snap, stored, empty, over;   // < 2^32 - 1 replies: no count wraps
};
__device__ __forceinline__ ret6 scan_op(const ret6& a, const ret6& b) {
    return ret6{a.tiles + b.tiles, a.bytes + b.bytes, a.snap + b.snap, a.stored + b.stored, a.empty + b.empty,
                a.over + b.over};
}

__device__ __forceinline__ uint64_t retain_replies(const retain_tables& t) {
    const uint64_t d = *t.nrep_dev;
    return d < t.rep_cap ? d : t.rep_cap;
}

// One thread per reply: the largest publishing reply per topic (win: zero on entry).
__global__ __launch_bounds__(256) void k_retain_pick(retain_tables in, uint32_t* __restrict__ win) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= retain_replies(in)) return;
    const uint32_t t = in.topic[i];
    if (in.kind[i] == RK_PUB && t < in.ntopics) atomicMax(&win[t], (uint32_t)i + 1u);
}

// What topic t holds once the turn's update has run: its winner's row where a
// reply published to it, the caller's entry otherwise (no winner writes that
// one).  Selects, no early return (the compiler note of hvws_route.hip).
__device__ __forceinline__ bool retained_after(const retain_tables& in, const uint32_t* win, uint32_t t, uint64_t& len,
                                               uint32_t& flags) {
    const bool topic_ok = t < in.ntopics;
    const uint32_t w = topic_ok ? win[t] : 0u;
    uint32_t set = 0;
    len = 0;
    flags = 0;
    if (w) {
        const dtxmsg r = in.rows[w - 1];
        len = r.len;
        flags = r.flags;
        set = 1;
    } else if (topic_ok) {
        const dretained e = in.ret[t];
        len = e.len;
        flags = e.flags;
        set = e.set;
    }
    return set == 1 && len > 0 && len <= in.slot;
}

// the topic a SUB reply names: the route pass moved it into its event
__device__ __forceinline__ uint32_t retain_sub_topic(const retain_tables& in, uint64_t i) {
    const uint64_t e = (uint64_t)in.rt_ex[4 * i + 1] + in.rt_ex[4 * i + 2];   // subscribes + unsubscribes before i
    return e < in.rep_cap ? in.ev[e].topic : ~0u;
}

struct retain_load {
    retain_tables in;
    const uint32_t* win;
    __device__ __forceinline__ ret6 operator()(uint64_t i) const {
        ret6 v{};
        if (i < retain_replies(in)) {
            const uint32_t k = in.kind[i];
            if (k == RK_PUB) {
                const uint32_t t = in.topic[i];
                const bool won = t < in.ntopics && win[t] == (uint32_t)i + 1u;
                const uint64_t len = in.rows[i].len;
                const bool stores = won && len > 0 && len <= in.slot;
                v.tiles = stores ? (len + RETAIN_TILE - 1) / RETAIN_TILE : 0;
                v.bytes = stores ? len : 0;
                v.stored = stores ? 1u : 0u;
                v.empty = won && len == 0 ? 1u : 0u;
                v.over = won && len > in.slot ? 1u : 0u;
            } else if (k == RK_SUB) {
                uint64_t len;
                uint32_t fl;
                v.snap = retained_after(in, win, retain_sub_topic(in, i), len, fl) ? 1u : 0u;
            }
        }
        return v;
    }
};

// One thread per reply and per segment (the grid covers the larger count).
__global__ __launch_bounds__(256) void k_retain_finish(retain_tables in, retain_work w, const ret6* __restrict__ ex,
                                                       const ret6* __restrict__ total) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nrep = retain_replies(in);
    const ret6 tot = *total;
    if (i == 0) {
        w.meta[0] = tot.snap;
        w.meta[1] = tot.stored;
        w.meta[2] = tot.empty;
        w.meta[3] = tot.over;
        w.meta[4] = tot.bytes;
        w.meta[5] = tot.snap;
        w.pl_tile[tot.stored] = tot.tiles;   // behind the last winner's tiles
    }
    if (i < in.nseg) {
        uint64_t a = in.rep_first[i], n = in.rep_count[i];
        if (a > nrep) a = nrep;
        if (n > nrep - a) n = nrep - a;
        const uint64_t ra = a < nrep ? ex[a].snap : tot.snap, rb = a + n < nrep ? ex[a + n].snap : tot.snap;
        w.first[i] = ra;
        w.count[i] = rb - ra;
    }
    if (i >= nrep) return;
    const uint32_t k = in.kind[i];
    const ret6 b = ex[i];
    if (k == RK_PUB) {
        const uint32_t t = in.topic[i];
        if (t < in.ntopics && w.win[t] == (uint32_t)i + 1u) {
            const dtxmsg r = in.rows[i];
            const bool stores = r.len > 0 && r.len <= in.slot;
            in.ret[t] = stores ? dretained{r.len, r.flags, 1u} : dretained{0, 0u, 0u};
            if (stores) {
                w.pl_tile[b.stored] = b.tiles;
                w.pl_src[b.stored] = r.off;
                w.pl_dst[b.stored] = (uint64_t)t * in.slot;
                w.pl_len[b.stored] = r.len;
            }
        }
    } else if (k == RK_SUB) {
        const uint32_t t = retain_sub_topic(in, i);
        uint64_t len;
        uint32_t fl;
        if (retained_after(in, w.win, t, len, fl)) {
            w.rows[b.snap] = dtxmsg{(uint64_t)t * in.slot, len, fl, 0u};
            w.topic[b.snap] = t;
            w.reply[b.snap] = i;
        }
    }
}

// The copy of the winning bodies into their slots, by destination tile (file
// comment).  total: the plan scan's total; pl_tile[0 .. stored]: the first tile
// of each stored winner and, behind the last, the tile count.
__global__ __launch_bounds__(RETAIN_T) void k_retain_copy(const uint8_t* __restrict__ out, uint64_t out_cap,
                                                          uint8_t* __restrict__ store,
                                                          const uint64_t* __restrict__ pl_tile,
                                                          const uint64_t* __restrict__ pl_src,
                                                          const uint64_t* __restrict__ pl_dst,
                                                          const uint64_t* __restrict__ pl_len,
                                                          const ret6* __restrict__ total) {
    const uint64_t tiles = total->tiles, ns = total->stored;
    const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * per;
    const uint64_t g1 = tiles - g0 < per ? tiles : g0 + per;
    if (g0 >= tiles || ns == 0) return;
    uint64_t w = 0, hi = ns;   // the last winner whose first tile is <= g0
    while (hi - w > 1) {
        const uint64_t mid = (w + hi) >> 1;
        if (pl_tile[mid] <= g0) w = mid;
        else hi = mid;
    }
    uint64_t first = pl_tile[w], next = pl_tile[w + 1];
    uint64_t src = pl_src[w], dst = pl_dst[w], len = pl_len[w];
    for (uint64_t g = g0; g < g1; ++g) {
        while (g >= next && w + 1 < ns) {   // every stored winner has a tile: one step per winner
            ++w;
            first = next;
            next = pl_tile[w + 1];
            src = pl_src[w];
            dst = pl_dst[w];
            len = pl_len[w];
        }
        const uint64_t c = (g - first) * RETAIN_TILE + (uint64_t)threadIdx.x * 16u;
        if (c >= len) continue;
        const uint32_t n = len - c < 16 ? (uint32_t)(len - c) : 16u;
        const u32x4 v = ld16_clipped(out, out_cap, src + c, n);
        uint8_t* d = store + dst + c;
        if (n == 16) {
            *reinterpret_cast<u32x4*>(d) = v;
        } else {   // the body's last partial chunk: no byte at or beyond len is written
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t b = 0; b < 15; ++b)
                if (b < n) d[b] = (uint8_t)(wd[b >> 2] >> (8u * (b & 3u)));
        }
    }
}

}  // namespace

uint64_t retain_scratch_bytes(uint64_t cap) { return (cap + 16 + scan_tmp_words(cap)) * sizeof(ret6); }

hipError_t launch_retain(const retain_tables& t, const retain_work& w, hipStream_t st) {
    ret6* ex = reinterpret_cast<ret6*>(w.scratch);
    ret6* total = ex + t.rep_cap;   // one value; 16 are set aside
    ret6* tmp = ex + t.rep_cap + 16;
    hipError_t e = hipSuccess;
    if (t.ntopics && (e = hipMemsetAsync(w.win, 0, (uint64_t)t.ntopics * 4, st)) != hipSuccess) return e;
    const uint64_t rb = (t.rep_cap + 255) / 256;
    if (rb) hipLaunchKernelGGL(k_retain_pick, dim3((uint32_t)rb), dim3(256), 0, st, t, w.win);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = launch_scan_of(retain_load{t, w.win}, ex, t.rep_cap, tmp, total, st);
    if (e != hipSuccess) return e;
    const uint64_t fb = std::max<uint64_t>(std::max<uint64_t>(rb, ((uint64_t)t.nseg + 255) / 256), 1);
    hipLaunchKernelGGL(k_retain_finish, dim3((uint32_t)fb), dim3(256), 0, st, t, w, ex, total);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the tile count is on the device alone: a grid that covers the most tiles
    // the turn can hold, at most RETAIN_GRID workgroups, each taking its share
    const uint64_t winners = std::min<uint64_t>(t.rep_cap, t.ntopics);
    if (winners == 0) return hipSuccess;
    const uint64_t most = winners + t.out_cap / RETAIN_TILE;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(most, RETAIN_GRID);
    hipLaunchKernelGGL(k_retain_copy, dim3(grid), dim3(RETAIN_T), 0, st, t.out, t.out_cap, t.store, w.pl_tile, w.pl_src,
                       w.pl_dst, w.pl_len, total);
    return hipGetLastError();
}

}  // namespace hvws
