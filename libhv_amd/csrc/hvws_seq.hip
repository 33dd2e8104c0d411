// hvws_seq.hip -- the kernels of hvws_sequence (include/hvws.h has the
// contract): every publication of the turn gets the next number of its topic,
// in table order, and the caller's counters move on by the turn's publications.
// The reference has no counterpart: its onmessage is user code.  Runs over what
// hvws_route left: topic and kind per reply.  A table pass: no payload byte is
// touched.
//
//   the pairs    one thread per reply slot: (key, value) = (topic, reply) for a
//                publication, (ntopics, reply) for every other slot, the slots
//                behind the reply count included.
//   the sort     launch_fan_sort, stable, fan_key_passes(ntopics) passes: each
//                topic's publications become one run, in table order, and the
//                slots that take no number the last run.
//   the heads    one device-wide scan over the sorted keys (the scan of
//                hvws_dev.h) of {position of the latest run head, runs of a
//                topic, publications}.  An element's rank in its topic is its
//                position minus its run head's; the total is the pass's totals.
//   the numbers  one thread per sorted element: seq[reply] = d_seq[topic] + 1 +
//                rank (0 for a slot that takes none).  d_seq is read only.
//   the counters a SEPARATE LATER kernel: each run's last element stores
//                d_seq[topic] += run length.  Fused with the numbers it would be
//                a race between workgroups: a run spans workgroups, and its
//                last element's store could land before another workgroup has
//                read the counter the run's numbers start from.  Between two
//                kernels of one stream it cannot.
//
// No atomic decides a number or a counter: the outputs are functions of the
// tables alone.  A topic without a publication is neither read nor written.
//
// Traffic per reply slot: 4 B topic + 1 B kind read, 8 B pair written; per sort
// pass 8 B read twice and 8 B written; 4 B key read by the scan, 16 B of scan
// state written and read twice, 8 B pair read twice, 8 B seq written; per
// publication 8 B of d_seq read, per topic published to 8 B read and written.
#include "hvws_dev.h"

namespace hvws {

namespace {

struct seq3 {
    uint64_t head;        // 1 + the position of the latest run head, 0: none yet
    uint32_t runs, pubs;  // runs of a topic, publications (< 2^32 - 1 replies: no count wraps)
};
__device__ __forceinline__ seq3 scan_op(const seq3& a, const seq3& b) {
    return seq3{a.head > b.head ? a.head : b.head, a.runs + b.runs, a.pubs + b.pubs};
}

__device__ __forceinline__ uint64_t seq_replies(const seq_tables& t) {
    const uint64_t d = *t.nrep_dev;
    return d < t.rep_cap ? d : t.rep_cap;
}

// One thread per reply slot.
__global__ __launch_bounds__(256) void k_seq_pairs(seq_tables t, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.rep_cap) return;
    const bool pub = i < seq_replies(t) && t.kind[i] == RK_PUB;
    const uint32_t tp = pub ? t.topic[i] : t.ntopics;
    key[i] = tp < t.ntopics ? tp : t.ntopics;   // hvws_route left no publication to a topic >= ntopics
    val[i] = (uint32_t)i;
}

// p begins a run of the sorted keys
__device__ __forceinline__ bool seq_is_head(const uint32_t* __restrict__ key, uint64_t p) {
    return p == 0 || key[p] != key[p - 1];
}

struct seq_load {
    const uint32_t* key;
    uint32_t ntopics;
    __device__ __forceinline__ seq3 operator()(uint64_t p) const {
        const bool head = seq_is_head(key, p), pub = key[p] < ntopics;
        return seq3{head ? p + 1 : 0, head && pub ? 1u : 0u, pub ? 1u : 0u};
    }
};

// the position of the head of the run p is in: ex is the scan before p
__device__ __forceinline__ uint64_t seq_head_of(const uint32_t* __restrict__ key, const seq3* __restrict__ ex, uint64_t p) {
    return seq_is_head(key, p) ? p : ex[p].head - 1;   // p is no head: a head stands before it
}

// One thread per sorted element.  Reads d_seq, writes none of it.
__global__ __launch_bounds__(256) void k_seq_number(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                    uint64_t n, uint32_t ntopics, const seq3* __restrict__ ex,
                                                    const uint64_t* __restrict__ d_seq, uint64_t* __restrict__ seq) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = key[p];
    uint64_t v = 0;
    if (k < ntopics) v = d_seq[k] + 1 + (p - seq_head_of(key, ex, p));   // modulo 2^64
    seq[val[p]] = v;
}

// One thread per sorted element (at least one thread); the last of each topic's
// run moves the counter on.  Launched behind k_seq_number (file comment).
__global__ __launch_bounds__(256) void k_seq_counters(const uint32_t* __restrict__ key, uint64_t n, uint32_t ntopics,
                                                      const seq3* __restrict__ ex, const seq3* __restrict__ total,
                                                      uint64_t* __restrict__ d_seq, uint64_t* __restrict__ meta) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) {
        const seq3 tot = *total;
        meta[0] = tot.pubs;
        meta[1] = tot.runs;
    }
    if (p >= n) return;
    const uint32_t k = key[p];
    const bool last = p + 1 == n || key[p + 1] != k;
    if (k < ntopics && last) d_seq[k] += p - seq_head_of(key, ex, p) + 1;
}

}  // namespace

uint64_t seq_scratch_bytes(uint64_t cap) { return (cap + 16 + scan_tmp_words(cap)) * sizeof(seq3); }

hipError_t launch_sequence(const seq_tables& t, const seq_work& w, hipStream_t st) {
    const uint64_t n = t.rep_cap;
    seq3* ex = reinterpret_cast<seq3*>(w.scratch);
    seq3* total = ex + n;   // one value; 16 are set aside
    seq3* tmp = ex + n + 16;
    const uint32_t nb = (uint32_t)std::max<uint64_t>((n + 255) / 256, 1);
    int cur = 0;
    if (n) {
        hipLaunchKernelGGL(k_seq_pairs, dim3(nb), dim3(256), 0, st, t, w.key[0], w.val[0]);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if ((e = launch_fan_sort(w.key, w.val, n, fan_key_passes(t.ntopics), w.hist, &cur, st)) != hipSuccess) return e;
    }
    hipError_t e = launch_scan_of(seq_load{w.key[cur], t.ntopics}, ex, n, tmp, total, st);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(k_seq_number, dim3(nb), dim3(256), 0, st, w.key[cur], w.val[cur], n, t.ntopics, ex, t.d_seq, w.seq);
    hipLaunchKernelGGL(k_seq_counters, dim3(nb), dim3(256), 0, st, w.key[cur], n, t.ntopics, ex, total, t.d_seq, w.meta);
    return hipGetLastError();
}

}  // namespace hvws
