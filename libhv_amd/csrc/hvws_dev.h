// hvws_dev.h -- device helpers shared by the discovery kernels
// (hvws_kernels.hip, hvws_sieve.hip): 16-byte header loads, the fixed-format
// header decode of http/websocket_parser.c:60-142 and frame-record stores.
#pragma once

#include "hvws_internal.h"

namespace hvws {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- helpers

__device__ __forceinline__ uint32_t rotr32(uint32_t x, uint32_t r) {
    r &= 31u;
    return r ? (x >> r) | (x << (32u - r)) : x;
}

// Key word for 4-byte aligned words of a payload whose first byte sits at
// absolute offset `pay_off` with mask phase `phase`: byte at address a uses
// mask[(a - pay_off + phase) & 3] (http/websocket_parser.c:175).
__device__ __forceinline__ uint32_t key_for_aligned(uint32_t key, uint64_t pay_off, uint32_t phase) {
    uint32_t rot = (phase - (uint32_t)pay_off) & 3u;
    return rotr32(key, 8u * rot);
}

__device__ __forceinline__ uint64_t ld64_guard(const uint8_t* rx, uint64_t rx_len, uint64_t a) {
    if (a + 8 <= rx_len) return *reinterpret_cast<const uint64_t*>(rx + a);
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (a + k < rx_len) v |= (uint64_t)rx[a + k] << (8 * k);
    return v;
}

// 16 bytes starting at arbitrary absolute offset q (bytes past rx_len read 0).
// Inside the buffer the three words are loaded unconditionally, so the loads
// issue together and cost one memory round trip: guarded one by one, each
// sat behind its own branch and wait -- three dependent round trips per
// header in the walks (k_sieve_link: ~1.9 us per hop on an idle chip).
__device__ __forceinline__ void ld16(const uint8_t* rx, uint64_t rx_len, uint64_t q, uint64_t& lo,
                                     uint64_t& hi) {
    const uint64_t a = q & ~7ull;
    const uint32_t sh = (uint32_t)(q & 7u) * 8u;
    uint64_t w0, w1, w2;
    if (a + 24 <= rx_len) {
        const uint64_t* p = reinterpret_cast<const uint64_t*>(rx + a);
        w0 = p[0];
        w1 = p[1];
        w2 = p[2];
    } else {
        w0 = ld64_guard(rx, rx_len, a);
        w1 = ld64_guard(rx, rx_len, a + 8);
        w2 = ld64_guard(rx, rx_len, a + 16);
    }
    lo = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0;
    hi = sh ? (w1 >> sh) | (w2 << (64u - sh)) : w1;
}

// 16 bytes starting at arbitrary offset p of a buffer of plen bytes (bytes
// past plen read 0; no load leaves the buffer).
__device__ __forceinline__ void ld16_any(const uint8_t* pay, uint64_t plen, uint64_t p, uint64_t& lo, uint64_t& hi) {
    const uint64_t a = p & ~15ull;
    const uint32_t s = (uint32_t)(p & 15u);
    if (a + 32 <= plen) {
        const u32x4 va = *reinterpret_cast<const u32x4*>(pay + a);
        const u32x4 vb = *reinterpret_cast<const u32x4*>(pay + a + 16);
        const uint64_t w0 = va.x | ((uint64_t)va.y << 32), w1 = va.z | ((uint64_t)va.w << 32);
        const uint64_t w2 = vb.x | ((uint64_t)vb.y << 32), w3 = vb.z | ((uint64_t)vb.w << 32);
        const uint64_t x0 = s < 8 ? w0 : w1, x1 = s < 8 ? w1 : w2, x2 = s < 8 ? w2 : w3;
        const uint32_t sh = (s & 7u) * 8u;
        lo = sh ? (x0 >> sh) | (x1 << (64u - sh)) : x0;
        hi = sh ? (x1 >> sh) | (x2 << (64u - sh)) : x1;
    } else {
        lo = hi = 0;
        for (int b = 0; b < 16; ++b) {
            const uint64_t q = p + b;
            const uint64_t v = q < plen ? pay[q] : 0;
            if (b < 8) lo |= v << (8 * b);
            else hi |= v << (8 * (b - 8));
        }
    }
}

// bytes s..s+15 of the 32-byte little-endian pair (a, b), s in [0, 16)
__device__ __forceinline__ u32x4 funnel16(u32x4 a, u32x4 b, uint32_t s) {
    const uint64_t w0 = a.x | ((uint64_t)a.y << 32), w1 = a.z | ((uint64_t)a.w << 32);
    const uint64_t w2 = b.x | ((uint64_t)b.y << 32), w3 = b.z | ((uint64_t)b.w << 32);
    const uint64_t x0 = s < 8 ? w0 : w1, x1 = s < 8 ? w1 : w2, x2 = s < 8 ? w2 : w3;
    const uint32_t sh = (s & 7u) * 8u;
    const uint64_t lo = sh ? (x0 >> sh) | (x1 << (64u - sh)) : x0;
    const uint64_t hi = sh ? (x1 >> sh) | (x2 << (64u - sh)) : x1;
    return u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}

// Bytes [s, s + n) of out, n in 1 .. 16, as the low bytes of a 16-byte value.
// No load leaves [s & ~15, s + n rounded up to 16), nor [0, out_cap)
// (hvws_retain.hip, hvws_envelope.hip).
__device__ __forceinline__ u32x4 ld16_clipped(const uint8_t* __restrict__ out, uint64_t out_cap, uint64_t s, uint32_t n) {
    const uint64_t a = s & ~15ull;
    const uint32_t sft = (uint32_t)(s & 15u);
    const bool two = sft + n > 16u;
    if (a + (two ? 32u : 16u) <= out_cap) {
        const u32x4 va = *reinterpret_cast<const u32x4*>(out + a);
        const u32x4 vb = two ? *reinterpret_cast<const u32x4*>(out + a + 16) : va;
        return sft ? funnel16(va, vb, sft) : va;
    }
    uint32_t wd[4] = {0, 0, 0, 0};   // the buffer ends inside the chunk's lines: byte by byte
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (b < n && s + b < out_cap) wd[b >> 2] |= (uint32_t)out[s + b] << (8u * (b & 3u));
    return u32x4{wd[0], wd[1], wd[2], wd[3]};
}

// OR bytes [0, b1 - b0) of the 16-byte little-endian value (vlo, vhi) into
// bytes [b0, b1) of the chunk (olo, ohi); 0 <= b0 < b1 <= 16.
__device__ __forceinline__ void put_bytes(uint64_t& olo, uint64_t& ohi, uint64_t vlo, uint64_t vhi, uint32_t b0,
                                          uint32_t b1) {
    const uint32_t n = b1 - b0;
    if (n < 8) {
        vlo &= ~0ull >> (64u - 8u * n);
        vhi = 0;
    } else if (n < 16) {
        vhi = n == 8 ? 0 : vhi & (~0ull >> (64u - 8u * (n - 8u)));
    }
    if (b0 >= 8) {
        vhi = vlo << (8u * (b0 - 8u));
        vlo = 0;
    } else if (b0) {
        vhi = (vhi << (8u * b0)) | (vlo >> (64u - 8u * b0));
        vlo <<= 8u * b0;
    }
    olo |= vlo;
    ohi |= vhi;
}

// ---- device-wide exclusive scan (block scans, scan of the block sums, add) ----
// Over any value type V whose V{} is the identity of an associative
// scan_op(earlier, later): uint64_t sums here (the transmit side's frame
// offsets, the sieve's ranks) and hvws_msg.hip's three-component records.
// 256-thread workgroups, 4 consecutive elements per thread (1024 per block).
// Workgroups of 1024 threads waited 125-200 us each for a CU with 16 free
// wave slots while a pipelined unmask held the device (the frame sieve's
// scans, profiles/r2o_raw), against ~5 us alone.
constexpr int SCAN_T = 256;
constexpr int SCAN_I = 4;
constexpr int SCAN_B = SCAN_T * SCAN_I;

__device__ __forceinline__ uint64_t scan_op(uint64_t a, uint64_t b) { return a + b; }

template <typename V>
struct scan_from_array {
    const V* in;
    __device__ __forceinline__ V operator()(uint64_t i) const { return in[i]; }
};

// out[i] = the scan of load(0 .. i - 1) within the element's block;
// block_sums[b] = the block's total.
template <typename V, typename LOAD>
__global__ __launch_bounds__(SCAN_T) void k_scan_blocks(LOAD load, V* __restrict__ out, uint64_t n,
                                                        V* __restrict__ block_sums, V* __restrict__ total_if_one) {
    __shared__ V s[SCAN_T];
    const uint32_t t = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * SCAN_B + (uint64_t)t * SCAN_I;
    V v[SCAN_I], sum = V{};
#pragma unroll
    for (int k = 0; k < SCAN_I; ++k) {
        v[k] = i0 + k < n ? load(i0 + k) : V{};
        sum = scan_op(sum, v[k]);
    }
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_T; d <<= 1) {
        const V a = t >= (unsigned)d ? s[t - d] : V{};
        __syncthreads();
        s[t] = scan_op(a, s[t]);
        __syncthreads();
    }
    V run = t ? s[t - 1] : V{};   // exclusive within the block
#pragma unroll
    for (int k = 0; k < SCAN_I; ++k) {
        if (i0 + k < n) out[i0 + k] = run;
        run = scan_op(run, v[k]);
    }
    if (t == SCAN_T - 1) {
        block_sums[blockIdx.x] = s[t];
        if (total_if_one) *total_if_one = s[t];   // one block: its sum is the total
    }
}

template <typename V>
__global__ __launch_bounds__(SCAN_T) void k_add_block_base(V* __restrict__ out, uint64_t n,
                                                           const V* __restrict__ block_base) {
    const uint64_t i0 = (uint64_t)blockIdx.x * SCAN_B + (uint64_t)threadIdx.x * SCAN_I;
    const V b = block_base[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_I; ++k)
        if (i0 + k < n) out[i0 + k] = scan_op(b, out[i0 + k]);
}

// out[i] = scan of load(0 .. i - 1), *total = scan of all n; tmp holds
// scan_tmp_words(n) values.  add_top = false leaves the last step to the
// caller: out[i] is then relative to its block of SCAN_B elements, whose base
// is tmp[ceil(n / SCAN_B) + i / SCAN_B] when n > SCAN_B (and V{} otherwise).
constexpr uint64_t scan_tmp_words(uint64_t n) { return 4 * ((n + SCAN_B - 1) / SCAN_B) + 64; }
template <typename V, typename LOAD>
hipError_t launch_scan_of(LOAD load, V* out, uint64_t n, V* tmp, V* total, hipStream_t st, bool add_top = true) {
    if (n == 0) return hipMemsetAsync(total, 0, sizeof(V), st);
    const uint64_t nb = (n + SCAN_B - 1) / SCAN_B;
    V* sums = tmp;
    V* base = tmp + nb;
    hipLaunchKernelGGL((k_scan_blocks<V, LOAD>), dim3((uint32_t)nb), dim3(SCAN_T), 0, st, load, out, n, sums,
                       nb == 1 ? total : (V*)nullptr);
    if (nb > 1) {
        hipError_t e = launch_scan_of(scan_from_array<V>{sums}, base, nb, tmp + 2 * nb, total, st);
        if (e != hipSuccess) return e;
        if (add_top) hipLaunchKernelGGL((k_add_block_base<V>), dim3((uint32_t)nb), dim3(SCAN_T), 0, st, out, n, base);
    }
    return hipGetLastError();
}

// ---- the send's wire size (hvws_send.hip, hvws_budget.hip) ----
// header bytes of a frame of n payload bytes (http/websocket_parser.c:189-205)
__host__ __device__ __forceinline__ uint64_t send_hdr(uint64_t n, uint32_t masked) {
    return 2u + (n < 126 ? 0u : (n <= 0xFFFFu ? 2u : 8u)) + (masked ? 4u : 0u);
}
// Frames and output bytes of one message of len bytes cut into fragments of F
// (WebSocketChannel.cpp:24-48): all fragments but the last have one size.
__host__ __device__ __forceinline__ void send_wire(uint64_t len, uint64_t F, uint32_t masked, uint64_t& frames,
                                                   uint64_t& bytes) {
    if (len <= F) {
        frames = 1;
        bytes = send_hdr(len, masked) + len;
        return;
    }
    frames = (len - 1) / F + 1;
    const uint64_t last = len - (frames - 1) * F, full = send_hdr(F, masked) + F;
    // (frames - 1) * full <= 15 * len: saturate where that could wrap
    bytes = (len >> 59) ? ~0ull : (frames - 1) * full + send_hdr(last, masked) + last;
}

struct hdr {
    uint64_t length;
    uint32_t hlen;
    uint32_t flags;
    uint32_t key;
    uint32_t viol;   // V_* classes this header violates (reported only if enabled)
};

__device__ __forceinline__ bool reserved_opcode(uint32_t op) { return (op >= 3 && op <= 7) || op >= 0xB; }

// Fixed-format header decode from its first 16 bytes (lo = bytes 0..7 LE).
// Layout per websocket_build_frame (http/websocket_parser.c:207-256):
// b0 = FIN<<7 | opcode, b1 = MASK<<7 | len7, then 0/2/8 big-endian length
// bytes, then the 4 key bytes if MASK.  RSV bits are dropped (Q1).
// V = false: no violation classes (viol = 0), for callers whose validation
// mask is 0 (invalid_bits drops them there anyway).
template <bool V = true>
__device__ __forceinline__ hdr parse_hdr(uint64_t lo, uint64_t hi) {
    hdr h;
    uint32_t b0 = (uint32_t)lo & 0xFFu;
    uint32_t b1 = (uint32_t)(lo >> 8) & 0xFFu;
    uint32_t len7 = b1 & 0x7Fu;
    bool m = (b1 & 0x80u) != 0;
    h.flags = (b0 & F_OPMASK) | ((b0 & 0x80u) ? F_FIN : 0u) | (m ? F_MASK : 0u);
    uint32_t ext = len7 == 126 ? 2u : (len7 == 127 ? 8u : 0u);
    h.hlen = 2u + ext + (m ? 4u : 0u);
    uint64_t len16 = (((lo >> 16) & 0xFFu) << 8) | ((lo >> 24) & 0xFFu);
    uint64_t len64 = __builtin_bswap64((lo >> 16) | (hi << 48));
    h.length = len7 < 126 ? (uint64_t)len7 : (len7 == 126 ? len16 : len64);
    uint32_t k0 = (uint32_t)(lo >> 16), k2 = (uint32_t)(lo >> 32), k8 = (uint32_t)(hi >> 16);
    h.key = m ? (ext == 0 ? k0 : (ext == 2 ? k2 : k8)) : 0u;
    const uint32_t op = b0 & F_OPMASK;
    if constexpr (V)
        h.viol = ((b0 & 0x70u) ? V_RSV : 0u) | (reserved_opcode(op) ? V_OPCODE : 0u) |
                 ((op & 8u) && (!(b0 & 0x80u) || h.length > 125) ? V_CONTROL : 0u) |
                 (ext == 8 && (h.length >> 63) ? V_LEN64 : 0u) |
                 ((ext == 2 && h.length < 126) || (ext == 8 && h.length <= 0xFFFFu) ? V_NONMIN : 0u) |
                 (m ? 0u : V_UNMASKED);
    else
        h.viol = 0u;
    return h;
}

struct frec {
    int64_t  hdr_off;   // segment-relative here; made absolute on store
    uint64_t pay_off;   // segment-relative
    uint64_t pay_len;
    uint64_t length;
    uint32_t key;
    uint32_t info;
};

__device__ __forceinline__ void store_frame(const dframes& fr, uint64_t idx, uint64_t seg_off, const frec& r) {
    if (idx >= fr.cap) return;   // table sized by an estimate (SCAN_SINGLE): the host re-emits if it overflowed
    uint32_t phase = (r.info >> 8) & 3u;
    bool masked = (r.info & F_MASK) != 0;
    uint64_t abs_pay = seg_off + r.pay_off;
    fr.hdr_off[idx] = r.hdr_off < 0 ? -1 : (int64_t)(seg_off + (uint64_t)r.hdr_off);
    fr.pay_off[idx] = abs_pay;
    fr.pay_len[idx] = r.pay_len;
    fr.length[idx] = r.length;
    fr.key[idx] = r.key;
    fr.keyrot[idx] = masked ? key_for_aligned(r.key, abs_pay, phase) : 0u;
    fr.info[idx] = r.info;
}

__device__ __forceinline__ uint32_t invalid_bits(uint32_t viol, uint32_t vmask) {
    const uint32_t v = viol & vmask & V_ALL;
    return v ? I_INVALID | (v << I_VSHIFT) : 0u;
}

__device__ __forceinline__ void hdr_complete(frec& r, const dcarry& st, uint64_t pay_off, uint32_t vmask) {
    r.info = (r.info & ~0xFFu & ~(3u << 8)) | (st.flags & 0xFFu) | I_HDR | invalid_bits(st.viol, vmask);
    r.pay_off = pay_off;
    r.pay_len = 0;
    r.length = st.length;
    r.key = (st.flags & F_MASK) ? st.mask : 0u;
}

__device__ __forceinline__ bool parse_at(const uint8_t* rx, uint64_t rx_len, uint64_t seg_off, uint64_t L,
                                         uint64_t q, hdr& h) {
    // true when the frame at segment offset q is whole inside [0, L)
    if (q >= L || L - q < 2) return false;
    uint64_t lo, hi;
    ld16(rx, rx_len, seg_off + q, lo, hi);
    h = parse_hdr(lo, hi);
    const uint64_t rq = L - q;
    return h.hlen <= rq && h.length <= rq - h.hlen;
}

__device__ __forceinline__ void whole_frame_rec(frec& v, uint64_t q, const hdr& h, uint32_t vmask) {
    v.hdr_off = (int64_t)q;
    v.pay_off = q + h.hlen;
    v.pay_len = h.length;
    v.length = h.length;
    v.key = h.key;
    v.info = h.flags | I_HDR | I_START | I_END | (h.length ? I_BODY : 0u) | invalid_bits(h.viol, vmask);
}

}  // namespace hvws
