// hvws_envelope.hip -- the kernels of hvws_envelope (include/hvws.h has the
// contract): every reply's outgoing bytes written once into a second device
// buffer, publications with the line `M<topic>[ <sender>]\n` in front, and the
// row table that points into it.  hvws_envelope_sequenced is the same pass with
// the line `M<topic>[ <sender>] #<seq>\n`: env_of, the plan's load and the
// finish take the form as a template parameter, the copy is plan-driven and
// serves both.  The reference has no counterpart: its
// onmessage is user code.  Runs over what hvws_route left: the routed rows,
// topic and kind per reply.
//
//   the plan     one device-wide scan over the replies (the scan of
//                hvws_dev.h) of {copy tiles, bytes of d_env spanned, bytes
//                written, publications, verbatim replies, plan entries}.  The
//                total is the pass's totals; the value before reply i is its
//                offset e_i and says where its plan entry goes.  No atomic
//                places a row or a byte.
//   the finish   one thread per reply: the row R'[i] (and its twin for
//                hvws_retain_enveloped, whose length is 0 where the body is
//                empty), the envelope's bytes (at most 23, sequenced 45, byte
//                stores) and,
//                where a body is to be copied, the reply's entry of the dense
//                copy plan.
//   the copy     the payload path.  Work is cut by destination tile of
//                ENV_TILE bytes, not by message: the grid's workgroups (one
//                wave each) take equal runs of consecutive tiles, each finds
//                its first entry by binary search over the plan's tile offsets
//                and walks on from there, loading the next entry a tile ahead.
//                A body's tiles begin at the 16-byte chunk its first byte falls
//                in (the chunk it shares with the envelope).  Per whole chunk
//                two aligned 16-byte loads of the source and a funnel shift --
//                one load where the phases agree -- then one 16-byte store;
//                byte stores for the chunk shared with the envelope and for
//                the body's last partial one.
//
// Traffic per reply: 24 B row + 4 B topic + 1 B kind (+ 8 B piece word, one
// piece and 4 B of dest_of with HVWS_ENV_SENDER, 8 B of seq when sequenced) read
// by the plan and again by
// the finish, 40 B of scan state written and read, two 24 B rows written; per
// copied reply 32 B of plan; per publication at most 23 B (45 B) of envelope.  Per
// body byte: one read (plus at most 31 B around the body) and one write.
#include "hvws_dev.h"

namespace hvws {

namespace {

constexpr uint32_t ENV_T = 64;   // threads per workgroup of the copy (one wave): one 16-byte chunk each per tile
static_assert(ENV_TILE == ENV_T * 16, "a tile is one chunk per thread");

struct env6 {
    uint64_t tiles, span, bytes;
    uint32_t pub, verb, ent, pad;   // < 2^32 - 1 replies: no count wraps
};
__device__ __forceinline__ env6 scan_op(const env6& a, const env6& b) {
    return env6{a.tiles + b.tiles, a.span + b.span, a.bytes + b.bytes, a.pub + b.pub, a.verb + b.verb, a.ent + b.ent, 0u};
}

__device__ __forceinline__ uint64_t env_replies(const env_tables& t) {
    const uint64_t d = *t.nrep_dev;
    return d < t.rep_cap ? d : t.rep_cap;
}

// decimal digits of v: 1 .. 10
__device__ __forceinline__ uint32_t env_digits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
           (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}

// the destination id of the connection reply i came from (all ones for a piece
// outside the batch, which the fan-out refuses)
__device__ __forceinline__ uint32_t env_sender(const env_tables& t, uint64_t i) {
    const uint64_t p = t.piece[i];
    const uint64_t np = t.mg_meta[2] < t.piece_cap ? t.mg_meta[2] : t.piece_cap;
    const uint32_t s = p < np ? t.pieces[p].seg : t.nseg;
    return s < t.nseg ? t.dest_of[s] : ~0u;
}

// decimal digits of v: 1 .. 20
__device__ __forceinline__ uint32_t env_digits64(uint64_t v) {
    uint32_t n = 1;
    uint64_t p = 10;
#pragma unroll
    for (uint32_t k = 0; k < 19; ++k) {
        n += v >= p ? 1u : 0u;
        p *= 10u;   // 10^19 < 2^64: no wrap within the loop's uses
    }
    return n;
}

// What reply i puts into d_env: h envelope bytes, then body bytes from src.
// Selects, no early return (the compiler note of hvws_route.hip).
struct env_reply {
    uint64_t src, body;
    uint32_t h, flags, key, topic, sender;
    bool pub, verb;
    uint64_t seq;   // SEQ alone
};
// SEQ: the sequenced line, whose number is t.seq[i]
template <bool SEQ>
__device__ __forceinline__ env_reply env_of(const env_tables& t, uint64_t i) {
    const dtxmsg r = t.rows[i];
    const uint32_t k = t.kind[i];
    env_reply o;
    o.pub = k == RK_PUB;
    o.verb = k == RK_OTHER;
    o.src = r.off;
    o.body = o.pub || o.verb ? r.len : 0;
    o.flags = r.flags;
    o.key = r.key;
    o.topic = t.topic[i];
    o.sender = t.sender && o.pub ? env_sender(t, i) : 0u;
    o.h = o.pub ? 2u + env_digits(o.topic) + (t.sender ? 1u + env_digits(o.sender) : 0u) : 0u;
    if constexpr (SEQ) {
        o.seq = o.pub ? t.seq[i] : 0;
        o.h += o.pub ? 2u + env_digits64(o.seq) : 0u;   // SP '#' digits
    } else {
        o.seq = 0;
    }
    return o;
}

template <bool SEQ>
struct env_load {
    env_tables in;
    __device__ __forceinline__ env6 operator()(uint64_t i) const {
        env6 v{};
        if (i < env_replies(in)) {
            const env_reply o = env_of<SEQ>(in, i);
            const uint64_t bytes = o.h + o.body;
            v.tiles = o.body ? ((o.h & 15u) + o.body + ENV_TILE - 1) / ENV_TILE : 0;
            v.span = (bytes + 15u) & ~15ull;
            v.bytes = bytes;
            v.pub = o.pub ? 1u : 0u;
            v.verb = o.verb ? 1u : 0u;
            v.ent = o.body ? 1u : 0u;
        }
        return v;
    }
};

// v in decimal at p[0 .. nd): a division by a constant is a multiplication
__device__ __forceinline__ void env_put_digits(uint8_t* p, uint32_t v, uint32_t nd) {
#pragma unroll
    for (uint32_t k = 0; k < 10; ++k) {
        if (k < nd) p[nd - 1 - k] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
}

// v in decimal at p[0 .. nd), nd <= 20: three words of at most 9 digits, so that
// the digits come from 32-bit arithmetic
__device__ __forceinline__ void env_put_digits64(uint8_t* p, uint64_t v, uint32_t nd) {
    const uint64_t q = v / 1000000000ull;
    uint32_t w0 = (uint32_t)(v - q * 1000000000ull);
    uint32_t w2 = (uint32_t)(q / 1000000000ull);
    uint32_t w1 = (uint32_t)(q - (uint64_t)w2 * 1000000000ull);
#pragma unroll
    for (uint32_t k = 0; k < 20; ++k) {
        uint32_t& w = k < 9 ? w0 : k < 18 ? w1 : w2;
        if (k < nd) p[nd - 1 - k] = (uint8_t)('0' + w % 10u);
        w /= 10u;
    }
}

// One thread per reply (at least one thread).
template <bool SEQ>
__global__ __launch_bounds__(256) void k_env_finish(env_tables in, env_work w, const env6* __restrict__ ex,
                                                    const env6* __restrict__ total) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        const env6 tot = *total;
        w.meta[0] = tot.pub;
        w.meta[1] = tot.verb;
        w.meta[2] = tot.bytes;
        w.meta[3] = tot.span;
        w.pl_tile[tot.ent] = tot.tiles;   // behind the last entry's tiles
    }
    if (i >= env_replies(in)) return;
    const env_reply o = env_of<SEQ>(in, i);
    const env6 b = ex[i];
    const uint64_t e = b.span, bytes = o.h + o.body;
    // the caller's env_cap covers every turn (hvws_envelope_bound); a reply that
    // would leave it all the same writes nothing
    const bool fits = e <= in.env_cap && bytes <= in.env_cap - e;
    w.rows[i] = dtxmsg{e, fits ? bytes : 0, o.flags, o.key};
    // hvws_retain_enveloped's rows: an empty body is an empty publication
    w.rrows[i] = dtxmsg{e, fits && o.body ? bytes : 0, o.flags, o.key};
    if (o.body) {
        w.pl_tile[b.ent] = b.tiles;
        w.pl_src[b.ent] = o.src;
        w.pl_dst[b.ent] = e + o.h;
        w.pl_len[b.ent] = fits ? o.body : 0;
    }
    if (o.pub && fits) {
        uint8_t* p = in.env + e;
        const uint32_t nt = env_digits(o.topic);
        p[0] = 'M';
        env_put_digits(p + 1, o.topic, nt);
        if constexpr (SEQ) {
            const uint32_t nq = env_digits64(o.seq);
            const uint32_t at = o.h - nq - 3u;   // the SP before '#'
            if (in.sender) {
                p[1 + nt] = ' ';
                env_put_digits(p + 2 + nt, o.sender, at - nt - 2u);
            }
            p[at] = ' ';
            p[at + 1] = '#';
            env_put_digits64(p + at + 2, o.seq, nq);
        } else {
            if (in.sender) {
                p[1 + nt] = ' ';
                env_put_digits(p + 2 + nt, o.sender, o.h - nt - 3u);
            }
        }
        p[o.h - 1] = 0x0Au;
    }
}

// The copy of the bodies behind their envelopes, by destination tile (file
// comment).  total: the plan scan's total; pl_tile[0 .. ent]: the first tile of
// each entry and, behind the last, the tile count.  Entry w's tiles begin at
// pl_dst[w] & ~15; no store leaves [pl_dst[w], pl_dst[w] + pl_len[w]).
__global__ __launch_bounds__(ENV_T) void k_env_copy(const uint8_t* __restrict__ out, uint64_t out_cap,
                                                    uint8_t* __restrict__ env, const uint64_t* __restrict__ pl_tile,
                                                    const uint64_t* __restrict__ pl_src,
                                                    const uint64_t* __restrict__ pl_dst,
                                                    const uint64_t* __restrict__ pl_len,
                                                    const env6* __restrict__ total) {
    const uint64_t tiles = total->tiles, ns = total->ent;
    const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * per;
    const uint64_t g1 = tiles - g0 < per ? tiles : g0 + per;
    if (g0 >= tiles || ns == 0) return;
    uint64_t w = 0, hi = ns;   // the last entry whose first tile is <= g0
    while (hi - w > 1) {
        const uint64_t mid = (w + hi) >> 1;
        if (pl_tile[mid] <= g0) w = mid;
        else hi = mid;
    }
    uint64_t first = pl_tile[w], next = pl_tile[w + 1];
    uint64_t src = pl_src[w], dst = pl_dst[w], len = pl_len[w];
    // The entry behind the current one is loaded a tile ahead of its use: a run
    // of short bodies is one entry per tile, and its cost is the chain of
    // dependent loads (plan, then body) that this takes the plan out of.
    uint64_t n_next = 0, n_src = 0, n_dst = 0, n_len = 0;
    if (w + 1 < ns) {
        n_next = pl_tile[w + 2];
        n_src = pl_src[w + 1];
        n_dst = pl_dst[w + 1];
        n_len = pl_len[w + 1];
    }
    for (uint64_t g = g0; g < g1; ++g) {
        if (g >= next && w + 1 < ns) {   // every entry has a tile: at most one step per tile
            ++w;
            first = next;
            next = n_next;
            src = n_src;
            dst = n_dst;
            len = n_len;
            if (w + 1 < ns) {
                n_next = pl_tile[w + 2];
                n_src = pl_src[w + 1];
                n_dst = pl_dst[w + 1];
                n_len = pl_len[w + 1];
            }
        }
        // the chunk at `a` bytes behind the body's first chunk holds body bytes [lo - ph, end - ph)
        const uint32_t ph = (uint32_t)(dst & 15u);
        const uint64_t a = (g - first) * ENV_TILE + (uint64_t)threadIdx.x * 16u;
        const uint64_t stop = ph + len;
        if (a >= stop || len == 0) continue;
        const uint64_t lo = a < ph ? ph : a;
        const uint64_t end = stop - a < 16 ? stop : a + 16;
        const uint32_t n = (uint32_t)(end - lo);
        const u32x4 v = ld16_clipped(out, out_cap, src + (lo - ph), n);
        uint8_t* d = env + (dst - ph) + lo;
        if (n == 16) {
            *reinterpret_cast<u32x4*>(d) = v;
        } else {   // shared with the envelope, or the body's last: no byte outside the body is written
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t b = 0; b < 15; ++b)
                if (b < n) d[b] = (uint8_t)(wd[b >> 2] >> (8u * (b & 3u)));
        }
    }
}

}  // namespace

uint64_t env_scratch_bytes(uint64_t cap) { return (cap + 16 + scan_tmp_words(cap)) * sizeof(env6); }

hipError_t launch_envelope(const env_tables& t, const env_work& w, hipStream_t st) {
    env6* ex = reinterpret_cast<env6*>(w.scratch);
    env6* total = ex + t.rep_cap;   // one value; 16 are set aside
    env6* tmp = ex + t.rep_cap + 16;
    const uint64_t fb = std::max<uint64_t>((t.rep_cap + 255) / 256, 1);
    hipError_t e;
    if (t.seq) {   // hvws_envelope_sequenced
        e = launch_scan_of(env_load<true>{t}, ex, t.rep_cap, tmp, total, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_env_finish<true>, dim3((uint32_t)fb), dim3(256), 0, st, t, w, ex, total);
    } else {
        e = launch_scan_of(env_load<false>{t}, ex, t.rep_cap, tmp, total, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_env_finish<false>, dim3((uint32_t)fb), dim3(256), 0, st, t, w, ex, total);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (t.rep_cap == 0) return hipSuccess;
    // the tile count is on the device alone: a grid that covers the most tiles
    // the turn can hold, at most ENV_GRID workgroups, each taking its share
    const uint64_t most = t.rep_cap + (t.out_cap + 15 * t.rep_cap) / ENV_TILE;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(most, ENV_GRID);
    hipLaunchKernelGGL(k_env_copy, dim3(grid), dim3(ENV_T), 0, st, t.out, t.out_cap, t.env, w.pl_tile, w.pl_src, w.pl_dst,
                       w.pl_len, total);
    return hipGetLastError();
}

}  // namespace hvws
