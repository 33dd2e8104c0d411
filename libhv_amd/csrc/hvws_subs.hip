// hvws_subs.hip -- the table kernels of hvws_subs_update (include/hvws.h has
// the contract): the next subscription table of hvws_fanout from the current
// one, a list of join / leave / drop events and the connections the last reply
// call closed -- what the reference's event loop does to its channel map
// (evpp/TcpServer.h removeChannel) one connection at a time.
//
// Stamps order everything: an old listing has stamp 0, the drop of a closed
// connection stamp 1, event e stamp e + 2.  A listing survives iff no LEAVE of
// its (topic, destination) pair and no DROP of its destination has a stamp at or
// above its own.
//
//   the drops        drop[d] = the last drop stamp of destination d: atomicMax
//                    over the closed segments, then over the DROP events.  A max
//                    does not depend on the order it is taken in.
//   the pairs        the events sorted stably by (topic, destination) with the
//                    sort of hvws_fan.hip: once by the destination's bits, then
//                    by the topic's, the second key gathered through the value.
//                    A DROP takes the topic `ntopics` and sorts behind every
//                    pair.  Within a pair the events keep their order, so the
//                    pair's last LEAVE is its last kill and the JOINs behind it
//                    are a suffix; a prefix count of the LEAVEs answers "is
//                    there a LEAVE in [a, b)" for any range.
//   the listings     one thread per old listing: its topic by binary search over
//                    d_topic_first (bounded by the rows of its workgroup's first
//                    and next workgroup's first listing, found once: brow), its pair
//                    by binary search over its topic's sorted events (evfirst[t]:
//                    where they begin); it survives iff drop[d] == 0 and its pair
//                    has no LEAVE, and marks its pair "listed before" (every
//                    writer stores the same value).
//   the joins        one thread per sorted event: a JOIN is effective iff no
//                    LEAVE follows it in its pair and drop[d] is below its
//                    stamp; under HVWS_SUBS_UNIQUE only the first of them, and
//                    none when the pair has no kill and was listed before.
//   the placement    two device scans (survive bits, effective bits), then
//                    new_first[t] = survivors before row t + effective joins of
//                    topics below t; a survivor goes to new_first[t] + its rank
//                    in the row, a join behind the row's survivors at its rank
//                    among the topic's joins -- the sorted order is the
//                    contract's (destination, event).  No atomics place anything.
//
// Traffic per old listing: 4 B read, the row and pair searches (cached words:
// two of brow, then the few rows that begin inside its workgroup and the
// topic's few events), 4 B of drop[], 1 B written, 8 B of
// rank written and read, 4 B written.  Per event: 12 B up, 8 B + 8 B per sort pass (hvws_fan.hip), 9 B of
// pair and kind, 16 B of ranks.
//
// hvws_subs_update_routed puts a merge in front of all that (launch_subs_merge):
// the event array is built on the device from the route pass's events, a DROP
// per closed or malformed segment, a DROP per OVER destination and the host's
// own events -- two compactions by the scan of hvws_dev.h and one append
// kernel; 12 B read and written per event, 2 B of flags and 8 B of rank per
// segment, 1 B and 8 B per destination.
#include "hvws_dev.h"

namespace hvws {

namespace {

constexpr uint32_t OP_JOIN = 1u, OP_LEAVE = 2u, OP_DROP = 3u;

// the first of pk[lo .. hi) that is >= x (hi when there is none)
__device__ __forceinline__ uint64_t subs_lower(const uint64_t* pk, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pk[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// an exclusive scan's value at i in [0, n]: the total stands behind the array
__device__ __forceinline__ uint64_t rank_at(const uint64_t* r, uint64_t n, const uint64_t* total, uint64_t i) {
    return i < n ? r[i] : *total;
}
// the row of listing k: the last t in [lo, hi) with first[t] <= k (empty rows
// share their successor's first and are passed over).  lo < hi <= ntopics.
__device__ __forceinline__ uint32_t subs_row(const uint64_t* first, uint32_t lo, uint32_t hi, uint64_t k) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}
// ... for a thread of a 256-thread workgroup over consecutive listings: brow
// (k_subs_brow) holds the row of every 256th listing, so the workgroup's rows
// lie between two neighbouring entries and a lane searches only the few rows
// that begin inside the workgroup's 256 listings.  A table that is not dense
// may give hi < lo: the result is some row of the table then, and the call fails.
__device__ __forceinline__ uint32_t subs_row_of(const uint64_t* first, const uint32_t* brow, uint64_t k) {
    const uint32_t lo = brow[blockIdx.x], hi = brow[blockIdx.x + 1];
    return subs_row(first, lo, (hi > lo ? hi : lo) + 1, k);
}

// drop[dest_of[s]] = 1 for every closed segment; ctr[0] counts the distinct
// destinations (the one writer per destination that finds a zero)
__global__ __launch_bounds__(256) void k_subs_closed(const uint8_t* __restrict__ rflags, const uint32_t* __restrict__ dest_of,
                                                     uint32_t nseg, uint32_t ndest, uint32_t* __restrict__ drop,
                                                     uint32_t* __restrict__ ctr) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg || !(rflags[s] & RF_CLOSED)) return;
    const uint32_t d = dest_of[s];
    if (d >= ndest) return;   // the host refused it
    if (atomicMax(&drop[d], 1u) == 0u) atomicAdd(&ctr[0], 1u);
}

// the first sort's pairs (destination, event) and the DROP stamps
__global__ __launch_bounds__(256) void k_subs_events(const dsubev* __restrict__ ev, uint64_t nev, uint32_t ndest,
                                                     uint32_t* __restrict__ drop, uint32_t* __restrict__ key,
                                                     uint32_t* __restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nev) return;
    const dsubev e = ev[i];
    const uint32_t d = e.dest < ndest ? e.dest : ndest - 1;   // the host refused any other
    key[i] = d;
    val[i] = (uint32_t)i;
    if (e.op == OP_DROP) atomicMax(&drop[d], (uint32_t)i + 2u);
}

__device__ __forceinline__ uint32_t subs_topic_key(const dsubev& e, uint32_t ntopics) {
    return e.op == OP_DROP || e.topic >= ntopics ? ntopics : e.topic;
}

// the second sort's key, through the first sort's value
__global__ __launch_bounds__(256) void k_subs_topic_keys(const dsubev* __restrict__ ev, uint64_t nev, uint32_t ntopics,
                                                         const uint32_t* __restrict__ val, uint32_t* __restrict__ key) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nev) return;
    key[i] = subs_topic_key(ev[val[i]], ntopics);
}

// the sorted events as (topic << 32 | destination) and their ops; listed = 0
__global__ __launch_bounds__(256) void k_subs_pairs(const dsubev* __restrict__ ev, uint64_t nev, uint32_t ntopics,
                                                    uint32_t ndest, const uint32_t* __restrict__ val,
                                                    uint64_t* __restrict__ pk, uint8_t* __restrict__ kind,
                                                    uint8_t* __restrict__ listed) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nev) return;
    const dsubev e = ev[val[i]];
    const uint32_t d = e.dest < ndest ? e.dest : ndest - 1;
    pk[i] = ((uint64_t)subs_topic_key(e, ntopics) << 32) | d;
    kind[i] = (uint8_t)e.op;
    listed[i] = 0;
}

// evfirst[t] = the first sorted event of topic t or above, t in [0, ntopics]
__global__ __launch_bounds__(256) void k_subs_evfirst(const uint64_t* __restrict__ pk, uint64_t nev, uint32_t ntopics,
                                                      uint64_t* __restrict__ evfirst) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > ntopics) return;
    evfirst[t] = subs_lower(pk, 0, nev, t << 32);
}

struct leave_load {
    const uint8_t* kind;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return kind[i] == OP_LEAVE ? 1u : 0u; }
};
struct bit_load {
    const uint8_t* bit;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return bit[i]; }
};

// ctr[1] |= 1 for a table that is not dense
__global__ __launch_bounds__(256) void k_subs_rows(const uint64_t* __restrict__ first, uint32_t ntopics, uint64_t nmember,
                                                   uint32_t* __restrict__ ctr) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > ntopics) return;
    bool bad = false;
    if (t == 0) bad = first[0] != 0 || first[ntopics] != nmember;
    if (t < ntopics) bad = bad || first[t] > first[t + 1];
    if (bad) atomicOr(&ctr[1], 1u);
}

// brow[b] = the row of listing min(256 b, nmember - 1), b in [0, ceil(nmember / 256)]
__global__ __launch_bounds__(256) void k_subs_brow(const uint64_t* __restrict__ first, uint32_t ntopics, uint64_t nmember,
                                                   uint64_t nb, uint32_t* __restrict__ brow) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb) return;
    const uint64_t k = b * 256u < nmember ? b * 256u : nmember - 1;
    brow[b] = subs_row(first, 0, ntopics, k);
}

struct subs_in {
    const uint64_t* first;
    const uint32_t* member;
    uint32_t ntopics;
    uint64_t nmember;
    uint32_t ndest;
    uint64_t nev;
    bool unique;
};

// One thread per old listing: surv[k], and its pair's "listed before".
__global__ __launch_bounds__(256) void k_subs_old(subs_in in, const uint32_t* __restrict__ drop,
                                                  const uint32_t* __restrict__ brow, const uint64_t* __restrict__ pk,
                                                  const uint64_t* __restrict__ evfirst,
                                                  const uint64_t* __restrict__ nleave,
                                                  const uint64_t* __restrict__ leaves, uint8_t* __restrict__ listed,
                                                  uint8_t* __restrict__ surv, uint32_t* __restrict__ ctr) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= in.nmember) return;
    const uint32_t d = in.member[k];
    if (d >= in.ndest || in.ntopics == 0) {
        surv[k] = 0;
        atomicOr(&ctr[1], 1u);
        return;
    }
    bool live = drop[d] == 0u;
    if (in.nev) {
        const uint32_t t = subs_row_of(in.first, brow, k);
        const uint64_t key = ((uint64_t)t << 32) | d;
        const uint64_t e0 = evfirst[t], e1 = evfirst[t + 1];   // the topic's events
        const uint64_t a = subs_lower(pk, e0, e1, key);
        if (a < e1 && pk[a] == key) {
            const uint64_t b = subs_lower(pk, a, e1, key + 1);
            if (rank_at(nleave, in.nev, leaves, b) != nleave[a]) live = false;
            listed[a] = 1;
        }
    }
    surv[k] = live ? 1 : 0;
}

// One thread per sorted event: eff[i] = 1 for a JOIN that adds a listing.
__global__ __launch_bounds__(256) void k_subs_joins(subs_in in, const uint32_t* __restrict__ drop,
                                                    const uint64_t* __restrict__ pk, const uint64_t* __restrict__ evfirst,
                                                    const uint8_t* __restrict__ kind, const uint32_t* __restrict__ val,
                                                    const uint64_t* __restrict__ nleave,
                                                    const uint64_t* __restrict__ leaves,
                                                    const uint8_t* __restrict__ listed, uint8_t* __restrict__ eff) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.nev) return;
    bool on = false;
    if (kind[i] == OP_JOIN) {
        const uint64_t key = pk[i];
        const uint32_t dr = drop[(uint32_t)key];
        const uint32_t t = (uint32_t)(key >> 32);   // < ntopics: a JOIN
        const uint64_t b = subs_lower(pk, i, evfirst[t + 1], key + 1);
        const uint64_t lb = rank_at(nleave, in.nev, leaves, b);
        // no LEAVE behind it in the pair, and the destination's last drop before it
        on = lb == rank_at(nleave, in.nev, leaves, i + 1) && dr < val[i] + 2u;
        if (on && in.unique) {
            const uint64_t a = subs_lower(pk, evfirst[t], i, key);
            // the effective JOINs are a suffix of the pair: the first has none before it
            if (i > a && kind[i - 1] == OP_JOIN && dr < val[i - 1] + 2u) on = false;
            if (dr == 0u && lb == nleave[a] && listed[a]) on = false;   // never killed, and listed before
        }
    }
    eff[i] = on ? 1 : 0;
}

// meta[0..5] = new nmember, kept, added, removed, destinations dropped as closed, bad
__global__ void k_subs_meta(const uint64_t* __restrict__ kept, const uint64_t* __restrict__ added, uint64_t nmember,
                            const uint32_t* __restrict__ ctr, uint64_t* __restrict__ meta) {
    const uint64_t k = *kept, a = *added;
    meta[0] = k + a;
    meta[1] = k;
    meta[2] = a;
    meta[3] = nmember - k;
    meta[4] = ctr[0];
    meta[5] = ctr[1];
}

// first_out[t] = survivors before row t + effective joins of topics below t
__global__ __launch_bounds__(256) void k_subs_first(subs_in in, const uint64_t* __restrict__ evfirst,
                                                    const uint64_t* __restrict__ srank, const uint64_t* __restrict__ kept,
                                                    const uint64_t* __restrict__ jrank, const uint64_t* __restrict__ added,
                                                    uint64_t* __restrict__ first_out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > in.ntopics) return;
    first_out[t] = rank_at(srank, in.nmember, kept, in.first[t]) + rank_at(jrank, in.nev, added, evfirst[t]);
}

__global__ __launch_bounds__(256) void k_subs_place_old(subs_in in, const uint32_t* __restrict__ brow,
                                                        const uint8_t* __restrict__ surv,
                                                        const uint64_t* __restrict__ srank,
                                                        const uint64_t* __restrict__ first_out, uint64_t newn,
                                                        uint32_t* __restrict__ member_out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= in.nmember || !surv[k]) return;
    const uint32_t t = subs_row_of(in.first, brow, k);
    const uint64_t at = first_out[t] + (srank[k] - srank[in.first[t]]);   // first[t] <= k < nmember
    if (at < newn) member_out[at] = in.member[k];
}

__global__ __launch_bounds__(256) void k_subs_place_join(subs_in in, const uint64_t* __restrict__ pk,
                                                         const uint8_t* __restrict__ eff, const uint64_t* __restrict__ srank,
                                                         const uint64_t* __restrict__ kept,
                                                         const uint64_t* __restrict__ jrank, uint64_t newn,
                                                         uint32_t* __restrict__ member_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.nev || !eff[i]) return;
    const uint64_t key = pk[i];
    const uint32_t t = (uint32_t)(key >> 32);   // < ntopics: a JOIN
    // behind every survivor up to the end of row t, and every join before this one
    const uint64_t at = rank_at(srank, in.nmember, kept, in.first[t + 1]) + jrank[i];
    if (at < newn) member_out[at] = (uint32_t)key;
}

inline dim3 grid_of(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// ---- the merge of hvws_subs_update_routed: four dense appends ----
// Segment s gives a DROP iff the reply call closed it or the route call found it
// malformed; destination d iff the budget call cut it.  Both are inlined into a
// scan functor and into k_subs_merge: values by selects, no early return
// (hvws_route.hip, route_kind, has the miscompile that shape met).
__device__ __forceinline__ uint64_t merge_seg_drop(const subs_merge& in, uint64_t s) {
    return ((in.rflags[s] & RF_CLOSED) | (in.rtflags[s] & RT_BAD)) != 0 ? 1u : 0u;
}
__device__ __forceinline__ uint64_t merge_over(const subs_merge& in, uint64_t d) {
    return (in.bflags[d] & BF_OVER) != 0 ? 1u : 0u;
}
struct merge_seg_load {
    subs_merge in;
    __device__ __forceinline__ uint64_t operator()(uint64_t s) const { return merge_seg_drop(in, s); }
};
struct merge_over_load {
    subs_merge in;
    __device__ __forceinline__ uint64_t operator()(uint64_t d) const { return merge_over(in, d); }
};

// One thread per route event, segment, destination and host event (the grid
// covers the largest of the four capacities): out = the route's events, the
// connection drops in segment order, the OVER drops in destination order, the
// host's events; meta[0..4] = the four counts and their sum.  srank / orank: the
// exclusive scans of the two predicates, nsd / nod their totals.
__global__ __launch_bounds__(256) void k_subs_merge(subs_merge in, const uint64_t* __restrict__ srank,
                                                    const uint64_t* __restrict__ nsd,
                                                    const uint64_t* __restrict__ orank,
                                                    const uint64_t* __restrict__ nod, dsubev* __restrict__ out,
                                                    uint64_t* __restrict__ meta) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t have = *in.rt_nev;
    const uint64_t nrt = have < in.rt_cap ? have : in.rt_cap;
    const uint64_t b1 = nrt, b2 = b1 + *nsd, b3 = b2 + *nod;
    if (i == 0) {
        meta[0] = nrt;
        meta[1] = *nsd;
        meta[2] = *nod;
        meta[3] = in.nev;
        meta[4] = b3 + in.nev;
    }
    if (i < nrt) out[i] = in.rt_ev[i];
    if (i < in.nseg && merge_seg_drop(in, i)) out[b1 + srank[i]] = dsubev{OP_DROP, 0u, in.dest_of[i]};
    if (i < in.nover && merge_over(in, i)) out[b2 + orank[i]] = dsubev{OP_DROP, 0u, (uint32_t)i};
    if (i < in.nev) out[b3 + i] = in.host_ev[i];
}

}  // namespace

uint64_t subs_merge_words(uint32_t nseg, uint32_t nover) {
    return (uint64_t)nseg + nover + 32 + scan_tmp_words(nseg > nover ? nseg : nover);
}

hipError_t launch_subs_merge(const subs_merge& t, uint64_t* scratch, dsubev* out, uint64_t* meta, hipStream_t st) {
    uint64_t* srank = scratch;
    uint64_t* nsd = srank + t.nseg;                   // one value each; 16 are set aside
    uint64_t* orank = nsd + 16;
    uint64_t* nod = orank + t.nover;
    uint64_t* tmp = nod + 16;
    hipError_t e = launch_scan_of(merge_seg_load{t}, srank, t.nseg, tmp, nsd, st);
    if (e != hipSuccess) return e;
    e = launch_scan_of(merge_over_load{t}, orank, t.nover, tmp, nod, st);
    if (e != hipSuccess) return e;
    const uint64_t n = std::max<uint64_t>(std::max<uint64_t>(t.rt_cap, t.nev), std::max<uint32_t>(t.nseg, t.nover));
    hipLaunchKernelGGL(k_subs_merge, grid_of(std::max<uint64_t>(n, 1)), dim3(256), 0, st, t, srank, nsd, orank, nod, out,
                       meta);
    return hipGetLastError();
}

uint64_t subs_rank_words(uint64_t n) { return n + 16 + scan_tmp_words(n); }
uint64_t subs_event_rank_words(uint64_t nev) { return 2 * nev + 16 + scan_tmp_words(nev); }

hipError_t launch_subs_count(const subs_tables& t, const subs_work& w, hipStream_t st) {
    const subs_in in{t.topic_first, t.member, t.ntopics, t.nmember, t.ndest, t.nev, t.unique};
    uint32_t* ctr = reinterpret_cast<uint32_t*>(w.meta + 8);
    hipError_t e = hipMemsetAsync(w.meta, 0, 10 * 8, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(w.drop, 0, (uint64_t)t.ndest * 4, st);
    if (e != hipSuccess) return e;
    if (t.dest_of && t.nseg)
        hipLaunchKernelGGL(k_subs_closed, grid_of(t.nseg), dim3(256), 0, st, t.rflags, t.dest_of, t.nseg, t.ndest, w.drop,
                           ctr);
    int cur = 0;
    uint64_t* nleave = w.erank;
    uint64_t* leaves = w.erank + t.nev;               // one value each; 8 are set aside
    uint64_t* jrank = w.erank + t.nev + 8;
    uint64_t* added = jrank + t.nev;
    uint64_t* etmp = added + 8;
    uint64_t* srank = w.lrank;
    uint64_t* kept = w.lrank + t.nmember;
    uint64_t* ltmp = kept + 16;
    if (t.nev) {
        hipLaunchKernelGGL(k_subs_events, grid_of(t.nev), dim3(256), 0, st, t.ev, t.nev, t.ndest, w.drop, w.key[0],
                           w.val[0]);
        e = launch_fan_sort(w.key, w.val, t.nev, fan_key_passes(t.ndest - 1), w.hist, &cur, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_subs_topic_keys, grid_of(t.nev), dim3(256), 0, st, t.ev, t.nev, t.ntopics, w.val[cur],
                           w.key[cur]);
        e = launch_fan_sort(w.key, w.val, t.nev, fan_key_passes(t.ntopics), w.hist, &cur, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_subs_pairs, grid_of(t.nev), dim3(256), 0, st, t.ev, t.nev, t.ntopics, t.ndest, w.val[cur],
                           w.pk, w.kind, w.listed);
    }
    hipLaunchKernelGGL(k_subs_evfirst, grid_of((uint64_t)t.ntopics + 1), dim3(256), 0, st, w.pk, t.nev, t.ntopics,
                       w.evfirst);
    e = launch_scan_of(leave_load{w.kind}, nleave, t.nev, etmp, leaves, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_subs_rows, grid_of((uint64_t)t.ntopics + 1), dim3(256), 0, st, t.topic_first, t.ntopics,
                       t.nmember, ctr);
    if (t.nmember && t.ntopics) {
        const uint64_t nb = (t.nmember + 255) / 256;
        hipLaunchKernelGGL(k_subs_brow, grid_of(nb + 1), dim3(256), 0, st, t.topic_first, t.ntopics, t.nmember, nb, w.brow);
    }
    if (t.nmember)
        hipLaunchKernelGGL(k_subs_old, grid_of(t.nmember), dim3(256), 0, st, in, w.drop, w.brow, w.pk, w.evfirst, nleave, leaves,
                           w.listed, w.surv, ctr);
    if (t.nev)
        hipLaunchKernelGGL(k_subs_joins, grid_of(t.nev), dim3(256), 0, st, in, w.drop, w.pk, w.evfirst, w.kind,
                           w.val[cur], nleave, leaves, w.listed, w.eff);
    e = launch_scan_of(bit_load{w.surv}, srank, t.nmember, ltmp, kept, st);
    if (e != hipSuccess) return e;
    e = launch_scan_of(bit_load{w.eff}, jrank, t.nev, etmp, added, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_subs_meta, dim3(1), dim3(1), 0, st, kept, added, t.nmember, ctr, w.meta);
    return hipGetLastError();
}

hipError_t launch_subs_place(const subs_tables& t, const subs_work& w, uint64_t newn, uint64_t* first_out,
                             uint32_t* member_out, hipStream_t st) {
    const subs_in in{t.topic_first, t.member, t.ntopics, t.nmember, t.ndest, t.nev, t.unique};
    const uint64_t* jrank = w.erank + t.nev + 8;
    const uint64_t* added = jrank + t.nev;
    const uint64_t* srank = w.lrank;
    const uint64_t* kept = w.lrank + t.nmember;
    hipLaunchKernelGGL(k_subs_first, grid_of((uint64_t)t.ntopics + 1), dim3(256), 0, st, in, w.evfirst, srank, kept,
                       jrank, added, first_out);
    if (t.nmember && newn)
        hipLaunchKernelGGL(k_subs_place_old, grid_of(t.nmember), dim3(256), 0, st, in, w.brow, w.surv, srank, first_out,
                           newn, member_out);
    if (t.nev && newn)
        hipLaunchKernelGGL(k_subs_place_join, grid_of(t.nev), dim3(256), 0, st, in, w.pk, w.eff, srank, kept, jrank, newn,
                           member_out);
    return hipGetLastError();
}

}  // namespace hvws
