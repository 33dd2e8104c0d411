// hvws_utf8.hip -- UTF-8 validation of text messages (RFC 6455 sec. 5.6 / 8.1,
// RFC 3629) over the frame table of the last scan.  include/hvws.h has the
// contract: the state machine, the 32-bit transition word of a byte string
// (nibble k = exit state for entry state k), the fold rules.
//
//   k_u8_tiles  the only pass over the payload bytes, read-only, 16-byte
//               loads, one workgroup per U8_TILE bytes of the batch.  For a
//               record of more than 6 payload bytes it evaluates, at every
//               payload byte from the record's 4th on, a predicate that reads
//               that byte and the 3 before it (same record), and ORs a
//               failure into the record's flag word.  Nothing is serial over
//               bytes: tiles of one long frame only share that flag.
//   k_u8_words  one lane per record: the plain state machine over a payload
//               of at most 6 bytes; otherwise the 8 entry states run over the
//               first 3 bytes (head), the exit state comes from the last 3
//               (tail), and the flag says whether everything between holds.
//   k_u8_fold   one wave per segment folds its records' words in order into
//               the connection's state word and the first rejecting record.
//
// Why three pieces fix the word of a payload d of n > 6 bytes: every entry
// state other than ACCEPT has reached ACCEPT or REJECT after 3 bytes, the
// predicate below pins every character boundary from byte 3 on whatever came
// before, and the exit state only depends on the last lead byte within the
// final 3 bytes.  tests/test_utf8_oracle.py restates this decomposition in
// Python and compares it with the plain machine.
//
// The predicate at byte i (b = d[i], p1..p3 the bytes before it), with a
// byte's class len = 0 continuation (80..BF), 1 ASCII, 2 / 3 / 4 a lead of
// that many bytes (C2..DF, E0..EF, F0..F4), 9 never legal (C0, C1, F5..FF),
// and ok2(p, q) = q may follow lead p as its second byte (80..BF, narrowed
// after E0, ED, F0, F4):
//   b a continuation: the nearest non-continuation among p1, p2, p3 must be a
//     lead long enough to reach b, with a legal second byte;
//   b anything else: b is legal, and the nearest non-continuation among p1,
//     p2, p3 (if any) starts a character that ends exactly before b.
#include "hvws_dev.h"

namespace hvws {

namespace {

constexpr int U8_T = 256, U8_U = 4;
static_assert((uint64_t)U8_T * U8_U * 16u == U8_TILE, "tile geometry");
constexpr int U8_MAXF = 512;   // records staged in LDS per tile

__device__ __forceinline__ uint32_t u8_step(uint32_t s, uint32_t b) {
    if (s == 0u) {
        if (b < 0x80u) return 0u;
        if (b < 0xC2u) return U8_REJECT;
        if (b < 0xE0u) return 1u;
        if (b == 0xE0u) return 3u;
        if (b == 0xEDu) return 4u;
        if (b < 0xF0u) return 2u;
        if (b == 0xF0u) return 5u;
        if (b < 0xF4u) return 6u;
        return b == 0xF4u ? 7u : U8_REJECT;
    }
    if (s > 7u) return U8_REJECT;
    const uint32_t lo = s == 3u ? 0xA0u : (s == 5u ? 0x90u : 0x80u);
    const uint32_t hi = s == 4u ? 0x9Fu : (s == 7u ? 0x8Fu : 0xBFu);
    if (b < lo || b > hi) return U8_REJECT;
    return s == 1u ? 0u : (s <= 4u ? 1u : 2u);
}

__device__ __forceinline__ uint32_t u8_len(uint32_t b) {
    return b < 0x80u ? 1u : b < 0xC0u ? 0u : b < 0xC2u ? 9u : b < 0xE0u ? 2u : b < 0xF0u ? 3u : b < 0xF5u ? 4u : 9u;
}

__device__ __forceinline__ bool u8_ok2(uint32_t p, uint32_t q) {
    const uint32_t lo = p == 0xE0u ? 0xA0u : (p == 0xF0u ? 0x90u : 0x80u);
    const uint32_t hi = p == 0xEDu ? 0x9Fu : (p == 0xF4u ? 0x8Fu : 0xBFu);
    return q >= lo && q <= hi;
}

// The predicate at positions [jlo, jhi) of the 16-byte chunk w (plain text);
// h holds the 3 bytes before the chunk in its bits 8-31.  True if any fails.
__device__ __forceinline__ bool u8_chunk_bad(const u32x4 w, const uint32_t h, const uint32_t jlo,
                                             const uint32_t jhi) {
    // ASCII all through (the 3 bytes before included): every position holds
    if (((w.x | w.y | w.z | w.w | (h >> 8)) & 0x80808080u) == 0u) return false;
    // The same over the bytes the asked positions read, [jlo - 3, jhi) of the
    // chunk: a chunk holding a frame boundary has header and key bytes around
    // its payload pieces, and would otherwise send its whole wave through the
    // per-byte path below.  hb: bit q = top bit of byte q of the 19-byte window.
    {
        auto top4 = [](uint32_t x) { return (((x >> 7) & 0x01010101u) * 0x01020408u) >> 24; };
        const uint32_t hb = (top4(h) >> 1) | (top4(w.x) << 3) | (top4(w.y) << 7) | (top4(w.z) << 11) | (top4(w.w) << 15);
        const uint32_t reads = ((1u << (jhi + 3u)) - 1u) & ~((1u << jlo) - 1u);   // jlo < jhi <= 16
        if ((hb & reads) == 0u) return false;
    }
    uint32_t B[19], L[19];
    B[0] = (h >> 8) & 0xFFu;
    B[1] = (h >> 16) & 0xFFu;
    B[2] = h >> 24;
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < 16; ++q) B[3 + q] = (ww[q >> 2] >> (8 * (q & 3))) & 0xFFu;
#pragma unroll
    for (int q = 0; q < 19; ++q) L[q] = u8_len(B[q]);
    bool P[18];   // P[q]: B[q + 1] may follow lead B[q]
#pragma unroll
    for (int q = 0; q < 18; ++q) P[q] = u8_ok2(B[q], B[q + 1]);
    uint32_t badm = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t l0 = L[j + 3], l1 = L[j + 2], l2 = L[j + 1], l3 = L[j];
        bool ok;
        if (l0 == 0u)
            ok = l1 != 0u ? (l1 >= 2u && l1 <= 4u && P[j + 2])
               : l2 != 0u ? (l2 >= 3u && l2 <= 4u && P[j + 1])
               : l3 != 0u ? (l3 == 4u && P[j])
                          : false;
        else
            ok = l0 != 9u && (l1 != 0u ? l1 == 1u : l2 != 0u ? l2 == 2u : l3 != 0u ? (l3 == 3u && P[j]) : true);
        badm |= ok ? 0u : (1u << j);
    }
    const uint32_t act = (jhi >= 16u ? 0xFFFFu : ((1u << jhi) - 1u)) & ~((1u << jlo) - 1u);
    return (badm & act) != 0u;
}

// One flag store per distinct record among the wave's failing lanes.
__device__ __forceinline__ void u8_report(bool bad, uint32_t rec, uint32_t* __restrict__ flags) {
    uint64_t m = __ballot(bad);
    const uint32_t lane = threadIdx.x & 63u;
    while (m) {
        const int l = __ffsll((unsigned long long)m) - 1;
        const uint32_t r = (uint32_t)__shfl((int)rec, l);
        const uint64_t same = __ballot(bad && rec == r);
        if (lane == (uint32_t)l) atomicOr(&flags[r], 1u);
        m &= ~same;
    }
}

template <typename OFF, typename END, typename KEY>
__device__ __forceinline__ void u8_chunk(const u32x4 v, const uint32_t h, const uint64_t c, const uint32_t k0,
                                         const uint32_t nf, OFF offf, END endf, KEY keyf, bool& bad, uint32_t& brec,
                                         uint32_t* __restrict__ flags) {
    uint32_t lo = 0, hi = nf;   // first record ending after c
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (endf(mid) > c) hi = mid;
        else lo = mid + 1;
    }
#pragma unroll 1
    for (uint32_t k = lo; k < nf; ++k) {
        const uint64_t o = offf(k), e = endf(k);
        if (o >= c + 16) break;
        // payload bytes of record k in the chunk, from the record's 4th byte on
        const uint64_t from = o + 3 > c ? o + 3 - c : 0;
        const uint32_t jlo = from > 16 ? 16u : (uint32_t)from;
        const uint32_t jhi = e < c + 16 ? (e > c ? (uint32_t)(e - c) : 0u) : 16u;
        if (jlo < jhi) {
            const uint32_t kw = keyf(k);
            if (u8_chunk_bad(v ^ u32x4{kw, kw, kw, kw}, h ^ kw, jlo, jhi)) {
                if (!bad) {
                    bad = true;
                    brec = k0 + k;
                } else if (brec != k0 + k) {   // a second failing record in one chunk
                    atomicOr(&flags[k0 + k], 1u);
                }
            }
        }
        if (e > c + 16) break;
    }
}

__global__ __launch_bounds__(U8_T) void k_u8_tiles(const uint8_t* __restrict__ rx, uint64_t rx_len,
                                                   const uint64_t* __restrict__ pay_off,
                                                   const uint64_t* __restrict__ pay_len,
                                                   const uint32_t* __restrict__ keyrot,
                                                   const uint32_t* __restrict__ tile_first,
                                                   const uint64_t* __restrict__ nfr_p, uint64_t cap, uint32_t masked,
                                                   uint32_t* __restrict__ flags) {
    constexpr int T = U8_T, U = U8_U;
    __shared__ uint64_t s_off[U8_MAXF];
    __shared__ uint64_t s_end[U8_MAXF];
    __shared__ uint32_t s_key[U8_MAXF];

    const uint64_t t = blockIdx.x;
    const uint64_t base = t * U8_TILE;
    const uint32_t tid = threadIdx.x;
    const uint64_t nfr = *nfr_p < cap ? *nfr_p : cap;
    const uint32_t k0 = tile_first[t];
    const uint32_t k1r = tile_first[t + 1];
    const uint32_t k1 = (uint64_t)k1r + 1 < nfr ? k1r + 1 : (uint32_t)nfr;
    const uint32_t nf = k1 > k0 ? k1 - k0 : 0u;
    if (nf == 0u) return;   // no payload byte in the tile

    const bool full = base + U8_TILE <= rx_len;
    u32x4 v[U];
    uint32_t h[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const uint64_t c = base + ((uint64_t)i * T + tid) * 16u;
        if (full || c + 16 <= rx_len) {
            v[i] = *reinterpret_cast<const u32x4*>(rx + c);
        } else {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            for (int b = 0; b < 16; ++b)
                if (c + b < rx_len) w[b >> 2] |= (uint32_t)rx[c + b] << (8 * (b & 3));
            v[i] = u32x4{w[0], w[1], w[2], w[3]};
        }
    }
    // the 3 bytes before each chunk: the neighbouring lane's last word, or a
    // re-read at the first lane of a wave
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const uint64_t c = base + ((uint64_t)i * T + tid) * 16u;
        uint32_t prev = (uint32_t)__shfl_up((int)v[i].w, 1);
        if ((tid & 63u) == 0u) prev = (c >= 16 && c <= rx_len) ? *reinterpret_cast<const uint32_t*>(rx + c - 4) : 0u;
        h[i] = prev;
    }

    const bool staged = nf <= (uint32_t)U8_MAXF;
    if (staged) {
        for (uint32_t i = tid; i < nf; i += T) {
            const uint64_t o = pay_off[k0 + i], n = pay_len[k0 + i];
            s_off[i] = o;
            s_end[i] = n > 6 ? o + n : o;   // short payloads are k_u8_words' alone: an empty span here
            s_key[i] = masked ? keyrot[k0 + i] : 0u;
        }
    }
    __syncthreads();

#pragma unroll
    for (int i = 0; i < U; ++i) {
        const uint64_t c = base + ((uint64_t)i * T + tid) * 16u;
        bool bad = false;
        uint32_t brec = 0u;
        if (c < rx_len) {
            if (staged)
                u8_chunk(
                    v[i], h[i], c, k0, nf, [&](uint32_t k) { return s_off[k]; }, [&](uint32_t k) { return s_end[k]; },
                    [&](uint32_t k) { return s_key[k]; }, bad, brec, flags);
            else
                u8_chunk(
                    v[i], h[i], c, k0, nf, [&](uint32_t k) { return pay_off[k0 + k]; },
                    [&](uint32_t k) {
                        const uint64_t n = pay_len[k0 + k];
                        return n > 6 ? pay_off[k0 + k] + n : pay_off[k0 + k];
                    },
                    [&](uint32_t k) { return masked ? keyrot[k0 + k] : 0u; }, bad, brec, flags);
        }
        u8_report(bad, brec, flags);
    }
}

__global__ __launch_bounds__(256) void k_u8_words(const uint8_t* __restrict__ rx, uint64_t rx_len,
                                                  const uint64_t* __restrict__ pay_off,
                                                  const uint64_t* __restrict__ pay_len,
                                                  const uint32_t* __restrict__ keyrot,
                                                  const uint64_t* __restrict__ nfr_p, uint64_t cap, uint32_t masked,
                                                  uint32_t* __restrict__ flags, uint32_t* __restrict__ words,
                                                  uint64_t* __restrict__ meta) {
    const uint64_t nfr = *nfr_p < cap ? *nfr_p : cap;
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) meta[0] = nfr;
    if (k >= nfr) return;
    const uint64_t o = pay_off[k], n = pay_len[k];
    const uint32_t kw = masked ? keyrot[k] : 0u;
    const uint32_t interior_bad = flags[k];
    if (interior_bad) flags[k] = 0u;   // the flag words are zero between passes
    if (o > rx_len || n > rx_len - o) {   // not a span of the batch: no scan writes one
        words[k] = 0xFFFFFFFFu;
        return;
    }
    auto byte_at = [&](uint64_t i) -> uint32_t {
        const uint64_t a = o + i;
        return ((uint32_t)rx[a] ^ (kw >> (8u * (uint32_t)(a & 3u)))) & 0xFFu;
    };
    uint32_t word = 0u;
    if (n <= 6) {
        uint32_t d[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = (uint64_t)i < n ? byte_at(i) : 0u;
#pragma unroll
        for (uint32_t e = 0; e < 8; ++e) {
            uint32_t s = e;
#pragma unroll
            for (int i = 0; i < 6; ++i)
                if ((uint64_t)i < n) s = u8_step(s, d[i]);
            word |= s << (4u * e);
        }
    } else {
        const uint32_t d0 = byte_at(0), d1 = byte_at(1), d2 = byte_at(2);
        const uint32_t t0 = byte_at(n - 3), t1 = byte_at(n - 2), t2 = byte_at(n - 1);
        uint32_t tail = 0u;   // 3 trailing continuations with the interior holding: a 4-byte character just ended
        if (u8_len(t2) != 0u) tail = u8_step(0u, t2);
        else if (u8_len(t1) != 0u) tail = u8_step(u8_step(0u, t1), t2);
        else if (u8_len(t0) != 0u) tail = u8_step(u8_step(u8_step(0u, t0), t1), t2);
#pragma unroll
        for (uint32_t e = 0; e < 8; ++e) {
            const uint32_t s = u8_step(u8_step(u8_step(e, d0), d1), d2);
            word |= ((s == U8_REJECT || interior_bad) ? U8_REJECT : tail) << (4u * e);
        }
    }
    words[k] = word;
}

// One record's effect on a connection's (state, text open) -- the fold rules
// of include/hvws.h.  REJECT stays REJECT through payloads and message ends.
__device__ __forceinline__ void u8_apply(uint32_t& st, uint32_t& text, uint32_t inf, uint32_t w) {
    const uint32_t op = inf & F_OPMASK;
    if (op >= 3u) return;   // control frames and reserved opcodes
    if ((inf & I_HDR) && op == 1u) {
        text = 1u;
        st = U8_ACCEPT;
    } else if ((inf & I_HDR) && op == 2u) {
        text = 0u;
        st = U8_ACCEPT;
    }
    if (text && (inf & I_BODY)) st = st > 7u ? U8_REJECT : (w >> (4u * st)) & 15u;
    if ((inf & I_END) && (inf & F_FIN) && text) {
        if (st != U8_ACCEPT) st = U8_REJECT;
        text = 0u;
    }
}

// One wave per segment, 64 records at a time, one per lane.  A text or binary
// frame header sets the state whatever it was, so the state after record j
// only depends on the records from the nearest such header at or before j (or
// from the state carried into the 64 when there is none): every lane replays
// that short chain -- its neighbours' records come by lane shuffle -- and the
// first lane that ends in REJECT is the verdict.  Up to that record no chain
// has seen a REJECT, so each equals the serial fold.  The trip count is the
// longest chain: 1 for unfragmented messages, at most 64.
__global__ __launch_bounds__(256) void k_u8_fold(const uint32_t* __restrict__ info, const uint32_t* __restrict__ words,
                                                 const uint64_t* __restrict__ meta,
                                                 const uint64_t* __restrict__ counts,
                                                 const uint64_t* __restrict__ bases, uint32_t nseg,
                                                 const uint32_t* __restrict__ state_in,
                                                 uint32_t* __restrict__ state_out, uint64_t* __restrict__ bad_out) {
    const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (s >= nseg) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nrec = meta[0];
    const uint64_t first = bases[s];
    uint64_t cnt = counts[s];
    if (first >= nrec) cnt = 0;
    else if (cnt > nrec - first) cnt = nrec - first;
    const uint32_t sw = state_in ? state_in[s] : 0u;
    uint32_t st = sw & 15u, text = (sw >> 4) & 1u;
    uint64_t bad = ~0ull;
    if (st > 7u) {   // REJECT carried in (8..14 are no states: the same): sticky, the segment's first record index
        st = U8_REJECT;
        bad = first;
        cnt = 0;
    }
    for (uint64_t b0 = 0; b0 < cnt && bad == ~0ull; b0 += 64) {
        const uint64_t left = cnt - b0;
        const uint32_t m = left < 64 ? (uint32_t)left : 64u;
        const uint32_t my_info = lane < m ? info[first + b0 + lane] : 8u;
        const uint32_t my_word = lane < m ? words[first + b0 + lane] : U8_IDENTITY;
        const uint32_t op = my_info & F_OPMASK;
        const bool reset = (my_info & I_HDR) && (op == 1u || op == 2u);
        const uint64_t below = __ballot(reset) & ((2ull << lane) - 1ull);   // headers at or before this lane
        const uint32_t r = below ? 63u - (uint32_t)__clzll((long long)below) : 0u;
        uint32_t lst = below ? U8_ACCEPT : st, ltext = below ? 0u : text;
        const uint32_t span = lane < m ? lane - r : 0u;
        for (uint32_t t = 0;; ++t) {
            const bool act = lane < m && t <= span;
            if (!__ballot(act)) break;
            const uint32_t src = r + t < 64u ? r + t : 63u;
            const uint32_t inf = (uint32_t)__shfl((int)my_info, (int)src);
            const uint32_t w = (uint32_t)__shfl((int)my_word, (int)src);
            if (act) u8_apply(lst, ltext, inf, w);
        }
        const uint64_t rej = __ballot(lane < m && lst == U8_REJECT);
        if (rej) {
            st = U8_REJECT;
            bad = first + b0 + (uint64_t)(__ffsll((unsigned long long)rej) - 1);
        } else {
            st = (uint32_t)__builtin_amdgcn_readlane((int)lst, (int)(m - 1u));
            text = (uint32_t)__builtin_amdgcn_readlane((int)ltext, (int)(m - 1u));
        }
    }
    if (st == U8_REJECT) text = 0u;   // one REJECT word, wherever the batch cuts fell
    if (lane == 0u) {
        state_out[s] = st | (text << 4);
        bad_out[s] = bad;
    }
}

}  // namespace

hipError_t launch_utf8(const uint8_t* rx, uint64_t rx_len, const uint64_t* pay_off, const uint64_t* pay_len,
                       const uint32_t* keyrot, const uint32_t* info, const uint64_t* nfr_dev, uint64_t cap,
                       const uint32_t* tile_first, uint64_t ntiles, int masked, uint32_t* flags, uint32_t* words,
                       uint64_t* meta, const uint64_t* counts, const uint64_t* bases, uint32_t nseg,
                       const uint32_t* state_in, uint32_t* state_out, uint64_t* bad, hipStream_t st) {
    if (ntiles)
        hipLaunchKernelGGL(k_u8_tiles, dim3((uint32_t)ntiles), dim3(U8_T), 0, st, rx, rx_len, pay_off, pay_len, keyrot,
                           tile_first, nfr_dev, cap, masked ? 1u : 0u, flags);
    const uint64_t wb = (cap + 255) / 256;
    hipLaunchKernelGGL(k_u8_words, dim3((uint32_t)(wb ? wb : 1)), dim3(256), 0, st, rx, rx_len, pay_off, pay_len, keyrot,
                       nfr_dev, cap, masked ? 1u : 0u, flags, words, meta);
    if (nseg)
        hipLaunchKernelGGL(k_u8_fold, dim3((nseg + 3) / 4), dim3(256), 0, st, info, words, meta, counts, bases, nseg,
                           state_in, state_out, bad);
    return hipGetLastError();
}

}  // namespace hvws
