// hvws_budget.hip -- the table kernels of hvws_budget (include/hvws.h has the
// contract): every destination's deliveries of the last hvws_fanout cut at that
// destination's byte budget, by hio_write's rule (event/nio.c:554-560: a write
// that would take write_bufsize above max_write_bufsize fails with
// ERR_OVER_LIMIT and the channel is closed), at message granularity.  No pass
// over the payload and no wait.
//
//   the size scan   one device-wide scan over the deliveries (the scan of
//                   hvws_dev.h) whose load functor computes each delivery's wire
//                   size from its row -- send_wire, the number the send's own
//                   message pass adds up -- so no size array is written.  S[k] is
//                   the wire bytes before delivery k, S[n] their total.
//   the cut         one thread per DESTINATION: a binary search over its range of
//                   S (increasing: sizes are positive) for the deliveries whose
//                   running sum stays within the budget.  It writes count2, the
//                   kept bytes and the flags; the destinations over are counted
//                   per wave (an atomic that counts, it places nothing).
//   two scans       over the destinations: first2 from count2, byte_off from the
//                   kept bytes, each with its total behind its last word.
//   the placement   one thread per DELIVERY: its destination is the sorted key
//                   the fan-out's sort left behind (key >> 1), its place
//                   first2[d] + (k - first[d]) when k - first[d] < count2[d].
//                   One destination holding every delivery spreads over the grid
//                   as a million destinations of one do.  A thread copies its whole
//                   24-byte row: three threads per row, 8 bytes each, measured
//                   slower.
//
// Traffic per delivery: 24 B read by the size scan, 8 B of S written and (above
// 1024 deliveries) read and written once more; by the placement 4 B of key, 24 B
// of row and 8 B of reply read, three 8-byte words of its destination (cached:
// neighbours share them) and 32 B written when kept.  Per destination: 16 B of
// first / count, 8 B of budget, ~log2(count) words of S, 17 B written by the cut;
// 16 B read and 16 B written by the two scans.
#include "hvws_dev.h"

namespace hvws {

namespace {

// What delivery k adds to the size scan.  maxlen: the message call's out_cap, the
// longest message a row of the table can name; the host checked that n messages
// of that length fit 64 bits, so the sum cannot wrap whatever the rows hold.
struct budget_load {
    const dtxmsg* rows;
    uint64_t F, maxlen;
    uint32_t masked;
    __device__ __forceinline__ uint64_t operator()(uint64_t k) const {
        const uint64_t len = rows[k].len;
        uint64_t fr, bytes;
        send_wire(len < maxlen ? len : maxlen, F, masked, fr, bytes);
        return bytes;
    }
};

// S: n + 1 words.  meta[3] (zero on entry) += the destinations over.
__global__ __launch_bounds__(256) void k_budget_cut(const uint64_t* __restrict__ S, uint64_t n,
                                                    const uint64_t* __restrict__ first,
                                                    const uint64_t* __restrict__ count, uint32_t ndest,
                                                    const uint64_t* __restrict__ budget, uint64_t budget_all,
                                                    uint64_t* __restrict__ count2, uint64_t* __restrict__ kept,
                                                    uint8_t* __restrict__ flags, unsigned long long* __restrict__ meta) {
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool over = false;
    if (d < ndest) {
        uint64_t a = first[d], cnt = count[d];
        if (a > n) a = n;   // the fan-out's ranges lie inside its table; no read leaves S whatever they hold
        if (cnt > n - a) cnt = n - a;
        const uint64_t b = budget ? budget[d] : budget_all, base = S[a];
        // the most deliveries m of the range with S[a + m] - base <= b (m = 0 always fits)
        uint64_t lo = 0, hi = cnt;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (S[a + mid] - base <= b) lo = mid;
            else hi = mid - 1;
        }
        over = lo < cnt;
        count2[d] = lo;
        kept[d] = S[a + lo] - base;
        flags[d] = over ? BF_OVER : 0u;
    }
    const uint64_t mo = __ballot(over);
    if ((threadIdx.x & 63u) == 0 && mo) atomicAdd(meta + 3, (unsigned long long)__popcll(mo));
}

// meta[0..2] = kept deliveries (the send's d_n), kept bytes, dropped deliveries
__global__ void k_budget_totals(const uint64_t* __restrict__ kept_del, const uint64_t* __restrict__ kept_bytes,
                                uint64_t n, uint64_t* __restrict__ meta) {
    const uint64_t k = *kept_del;
    meta[0] = k;
    meta[1] = *kept_bytes;
    meta[2] = n - k;
}

// key[k] >> 1: delivery k's destination (launch_fan_deliver's sorted keys)
__global__ __launch_bounds__(256) void k_budget_place(const uint32_t* __restrict__ key, uint64_t n, uint32_t ndest,
                                                      const uint64_t* __restrict__ first,
                                                      const uint64_t* __restrict__ count2,
                                                      const uint64_t* __restrict__ first2,
                                                      const dtxmsg* __restrict__ rows, const uint64_t* __restrict__ reply,
                                                      dtxmsg* __restrict__ out, uint64_t* __restrict__ reply_out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t d = key[k] >> 1;
    if (d >= ndest) return;
    const uint64_t a = first[d];
    if (k < a || k - a >= count2[d]) return;
    const uint64_t at = first2[d] + (k - a);   // <= k: the kept deliveries before it are no more than the deliveries
    if (at >= n) return;
    out[at] = rows[k];
    reply_out[at] = reply[k];
}

}  // namespace

uint64_t budget_scratch_words(uint64_t n, uint32_t ndest) {
    return n + 16 + scan_tmp_words(n > ndest ? n : ndest);
}

uint64_t budget_wire(uint64_t len, uint64_t F, int masked) {
    uint64_t fr, bytes;
    send_wire(len, F, masked ? 1u : 0u, fr, bytes);
    return bytes;
}

hipError_t launch_budget(const budget_tables& t, const budget_work& w, hipStream_t st) {
    uint64_t* S = w.scratch;            // n + 1 words (16 are set aside behind the n)
    uint64_t* tmp = w.scratch + t.n + 16;
    hipError_t e = hipMemsetAsync(w.meta, 0, 64, st);
    if (e != hipSuccess) return e;
    e = launch_scan_of(budget_load{t.rows, t.F, t.maxlen, t.masked ? 1u : 0u}, S, t.n, tmp, S + t.n, st);
    if (e != hipSuccess) return e;
    const uint32_t db = (t.ndest + 255) / 256;
    hipLaunchKernelGGL(k_budget_cut, dim3(db), dim3(256), 0, st, S, t.n, t.first, t.count, t.ndest, t.budget, t.budget_all,
                       w.count2, w.kept, w.flags, reinterpret_cast<unsigned long long*>(w.meta));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan_of(scan_from_array<uint64_t>{w.count2}, w.first2, t.ndest, tmp, w.first2 + t.ndest, st);
    if (e != hipSuccess) return e;
    e = launch_scan_of(scan_from_array<uint64_t>{w.kept}, w.byte_off, t.ndest, tmp, w.byte_off + t.ndest, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_budget_totals, dim3(1), dim3(1), 0, st, w.first2 + t.ndest, w.byte_off + t.ndest, t.n, w.meta);
    if (t.n)
        hipLaunchKernelGGL(k_budget_place, dim3((uint32_t)((t.n + 255) / 256)), dim3(256), 0, st, t.key, t.n, t.ndest,
                           t.first, w.count2, w.first2, t.rows, t.reply, w.out, w.reply_out);
    return hipGetLastError();
}

}  // namespace hvws
