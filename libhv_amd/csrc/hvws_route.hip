// hvws_route.hip -- the table kernels of hvws_route (include/hvws.h has the
// contract): every TEXT / BINARY reply of hvws_replies classified by the
// command header its message begins with -- publish, subscribe, unsubscribe or
// malformed -- into a topic per reply, the reply rows with the header trimmed
// off, and the dense list of join / leave events.  The reference has no
// counterpart: its onmessage is user code.  At most 12 bytes per reply are read
// where the message call left them; no pass over the payload.
//
//   the parse    one thread per reply: min(len, 12) bytes at any alignment,
//                clipped to the message (whole dwords where four bytes are
//                left, then a byte tail), the grammar, the row / topic / kind
//                as if no connection failed, and for a malformed message an
//                atomicMin of the reply index on its segment's word: a
//                minimum, so the order the threads run in does not show.
//   the count    one device-wide scan over the replies (the scan of
//                hvws_dev.h) of {publications, subscribes, unsubscribes,
//                bad + stopped}, each reply's final kind formed on the way:
//                a data reply behind its segment's first malformed one is
//                STOPPED.  The scan's total is the pass's totals; its value
//                before reply i says where i's event goes.  No atomic places
//                an event.
//   the finish   one thread per reply: STOPPED replies get their row back and
//                lose their topic, SUB / UNSUB replies write their event and
//                give up the topic word that carried the id this far; one
//                thread per segment: flags.
//
// Traffic per reply: its 24 B row, 8 B piece word and 24 B piece read, one
// line of the message bytes touched; 24 + 4 + 1 B written by the parse, 16 B
// of scan state written and read, and 12 B per event.
#include "hvws_dev.h"

namespace hvws {

namespace {

struct route4 {
    uint32_t pub, sub, unsub, bad;   // < 2^32 - 1 replies: no sum wraps
};
__device__ __forceinline__ route4 scan_op(const route4& a, const route4& b) {
    return route4{a.pub + b.pub, a.sub + b.sub, a.unsub + b.unsub, a.bad + b.bad};
}

constexpr uint32_t ROUTE_NONE32 = 0xFFFFFFFFu;
constexpr uint32_t ROUTE_HDR = 12;   // HVWS_ROUTE_HDR_MAX

__device__ __forceinline__ uint64_t route_replies(const route_tables& t) {
    const uint64_t d = *t.nrep_dev;
    return d < t.rep_cap ? d : t.rep_cap;
}
// the segment of the piece reply i answers (nseg for a piece outside the batch)
__device__ __forceinline__ uint32_t route_seg(const route_tables& t, uint64_t i) {
    const uint64_t p = t.piece[i];
    const uint64_t np = t.mg_meta[2] < t.piece_cap ? t.mg_meta[2] : t.piece_cap;
    if (p >= np) return t.nseg;
    const uint32_t s = t.pieces[p].seg;
    return s < t.nseg ? s : t.nseg;
}
__device__ __forceinline__ bool route_data(uint32_t flags) {
    const uint32_t op = flags & F_OPMASK;
    return op == 1 || op == 2;
}

// The grammar over bytes [0, n) of a message of L bytes, n = min(L, 12) (less
// where the output buffer ends first), packed little-endian in w[0..2]:
// verb, digits, LF.  Returns the kind; id and h are set for PUB / SUB / UNSUB.
__device__ __forceinline__ uint32_t route_parse(const uint32_t w[3], uint32_t n, uint64_t L, uint32_t ntopics,
                                                uint32_t& id, uint32_t& h) {
    auto byte = [&](uint32_t k) { return (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu; };
    id = ROUTE_NONE32;
    h = 0;
    if (n < 3) return RK_BAD;   // the shortest header is verb, digit, LF
    const uint32_t verb = byte(0);
    if (verb != 'P' && verb != 'S' && verb != 'U') return RK_BAD;
    uint64_t v = 0;
    uint32_t nd = 0;
    // at most ten digits: an eleventh stands where the LF had to be
    while (nd < 10 && 1 + nd < n) {
        const uint32_t c = byte(1 + nd);
        if (c < '0' || c > '9') break;
        v = v * 10 + (c - '0');
        ++nd;
    }
    if (nd == 0) return RK_BAD;
    if (nd > 1 && byte(1) == '0') return RK_BAD;   // a leading zero
    if (1 + nd >= n || byte(1 + nd) != 0x0Au) return RK_BAD;
    if (v >= ntopics) return RK_BAD;               // in 64 bits: ten digits exceed 2^32
    if (verb != 'P' && L != nd + 2) return RK_BAD;   // bytes behind a command's LF
    h = nd + 2;
    id = (uint32_t)v;
    return verb == 'P' ? RK_PUB : verb == 'S' ? RK_SUB : RK_UNSUB;
}

// One thread per reply: row, topic and kind as if no connection failed (topic
// carries the id of SUB / UNSUB replies until the finish), and the first
// malformed reply per segment (first_bad: all ones on entry).
__global__ __launch_bounds__(256) void k_route_parse(route_tables in, dtxmsg* __restrict__ rows,
                                                     uint32_t* __restrict__ topic, uint8_t* __restrict__ kind,
                                                     unsigned long long* __restrict__ first_bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= route_replies(in)) return;
    dtxmsg r = in.rep[i];
    uint32_t k = RK_OTHER, id = ROUTE_NONE32;
    if (route_data(r.flags)) {
        // bytes [off, off + n): inside the message and inside the output
        uint32_t n = r.len < ROUTE_HDR ? (uint32_t)r.len : ROUTE_HDR;
        if (r.off >= in.out_cap) n = 0;
        else if (in.out_cap - r.off < n) n = (uint32_t)(in.out_cap - r.off);
        const uint8_t* p = in.out + r.off;
        uint32_t w[3] = {0, 0, 0};
        const uint32_t full = n >> 2;
#pragma unroll
        for (uint32_t q = 0; q < 3; ++q)
            if (q < full) __builtin_memcpy(&w[q], p + 4 * q, 4);   // an unaligned dword load
        for (uint32_t b = 4 * full; b < n; ++b) w[b >> 2] |= (uint32_t)p[b] << (8u * (b & 3u));
        uint32_t h;
        k = route_parse(w, n, r.len, in.ntopics, id, h);
        if (k == RK_PUB) {
            r.off += h;
            r.len -= h;
        } else {
            const uint32_t s = route_seg(in, i);
            if (s >= in.nseg) {   // none of the batch's connections: no event can name it
                k = RK_BAD;
                id = ROUTE_NONE32;
            } else if (k == RK_BAD) {
                atomicMin(&first_bad[s], (unsigned long long)i);
            }
        }
    }
    rows[i] = r;
    topic[i] = id;
    kind[i] = (uint8_t)k;
}

// Reply i's kind once its segment's first malformed reply is known.
__device__ __forceinline__ uint32_t route_kind(const route_tables& in, const uint8_t* kind,
                                               const unsigned long long* first_bad, uint64_t i) {
    const uint32_t k = kind[i];
    const uint32_t s = route_seg(in, i);
    // a later malformed message is STOPPED like any other.  Selects, no early
    // return: with `if (k == RK_OTHER) return k;` in front, hipcc (ROCm 7.2) made
    // every data reply of k_route_finish STOPPED whatever the comparison gave.
    const unsigned long long b = s < in.nseg ? first_bad[s] : ~0ull;
    return k != RK_OTHER && b < i ? RK_STOPPED : k;
}

struct route_load {
    route_tables in;
    const uint8_t* kind;
    const unsigned long long* first_bad;
    __device__ __forceinline__ route4 operator()(uint64_t i) const {
        if (i >= route_replies(in)) return route4{};
        const uint32_t k = route_kind(in, kind, first_bad, i);
        return route4{k == RK_PUB ? 1u : 0u, k == RK_SUB ? 1u : 0u, k == RK_UNSUB ? 1u : 0u,
                      k == RK_BAD || k == RK_STOPPED ? 1u : 0u};
    }
};

// One thread per reply and per segment (the grid covers the larger count).
__global__ __launch_bounds__(256) void k_route_finish(route_tables in, const route4* __restrict__ ex,
                                                      const route4* __restrict__ total, dtxmsg* __restrict__ rows,
                                                      uint32_t* __restrict__ topic, uint8_t* __restrict__ kind,
                                                      const unsigned long long* __restrict__ first_bad,
                                                      uint8_t* __restrict__ flags, dsubev* __restrict__ ev,
                                                      uint64_t* __restrict__ meta) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        const route4 t = *total;
        meta[0] = (uint64_t)t.sub + t.unsub;
        meta[1] = t.pub;
        meta[2] = t.sub;
        meta[3] = t.unsub;
        meta[4] = t.bad;
    }
    if (i < in.nseg) flags[i] = first_bad[i] != ~0ull ? (uint8_t)RT_BAD : (uint8_t)0;
    if (i >= route_replies(in)) return;
    const uint32_t k = route_kind(in, kind, first_bad, i);
    if (k == RK_STOPPED) {
        rows[i] = in.rep[i];
        topic[i] = ROUTE_NONE32;
        kind[i] = (uint8_t)RK_STOPPED;
    } else if (k == RK_SUB || k == RK_UNSUB) {
        const route4 b = ex[i];
        const uint32_t s = route_seg(in, i);   // < nseg: the parse made anything else BAD
        ev[(uint64_t)b.sub + b.unsub] = dsubev{k == RK_SUB ? 1u : 2u, topic[i], in.dest_of[s < in.nseg ? s : 0]};
        topic[i] = ROUTE_NONE32;
    }
}

}  // namespace

uint64_t route_scratch_bytes(uint64_t cap) { return (cap + 16 + scan_tmp_words(cap)) * sizeof(route4); }

hipError_t launch_route(const route_tables& t, const route_work& w, hipStream_t st) {
    route4* ex = reinterpret_cast<route4*>(w.scratch);
    route4* total = ex + t.rep_cap;   // one value; 16 are set aside
    route4* tmp = ex + t.rep_cap + 16;
    unsigned long long* first_bad = reinterpret_cast<unsigned long long*>(w.bad_reply);
    hipError_t e = hipSuccess;
    if (t.nseg && (e = hipMemsetAsync(first_bad, 0xFF, (uint64_t)t.nseg * 8, st)) != hipSuccess) return e;
    const uint64_t rb = (t.rep_cap + 255) / 256;
    if (rb) hipLaunchKernelGGL(k_route_parse, dim3((uint32_t)rb), dim3(256), 0, st, t, w.rows, w.topic, w.kind, first_bad);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = launch_scan_of(route_load{t, w.kind, first_bad}, ex, t.rep_cap, tmp, total, st);
    if (e != hipSuccess) return e;
    const uint64_t fb = std::max<uint64_t>(std::max<uint64_t>(rb, ((uint64_t)t.nseg + 255) / 256), 1);
    hipLaunchKernelGGL(k_route_finish, dim3((uint32_t)fb), dim3(256), 0, st, t, ex, total, w.rows, w.topic, w.kind,
                       first_bad, w.flags, w.ev, w.meta);
    return hipGetLastError();
}

}  // namespace hvws
