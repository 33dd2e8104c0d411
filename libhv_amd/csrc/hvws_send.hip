// hvws_send.hip -- the table kernels of hvws_send_messages and hvws_replies
// (include/hvws.h has both contracts).
//
// hvws_send_messages is the reference's WebSocketChannel::send
// (http/WebSocketChannel.cpp:5-48) for a batch of messages whose lengths may
// exist only on the device.  Two table passes, no pass of their own over the
// payload (the bytes go through hvws_tx.hip's tile index and k_build):
//
//   the message pass  one device-wide scan over the messages (the scan of
//                     hvws_dev.h) carries three quantities at once:
//                       frames  ceil(len / F) per message (1 for len <= F)
//                       bytes   (frames - 1) * (hdr(F) + F) + hdr(last) + last:
//                               all fragments but the last have one size
//                       bad     messages outside the payload or with a flag
//                               bit outside 0x1F (they add nothing else)
//                     all saturating.  k_send_msgs then writes each message's
//                     first frame index, d_msg_off, the totals the host waits
//                     for, and whether the frames form a uniform layout (every
//                     message one frame of one length at a constant payload
//                     step: k_build then needs no tile index).
//   the expansion     one thread per FRAME: frame f finds its message by
//                     binary search over the first-frame table and writes the
//                     rows k_build reads.  Its output offset is the message's
//                     base plus j * (hdr(F) + F): no second scan.  One long
//                     message between a million short ones spreads over the
//                     grid as evenly as the reverse.
//
// hvws_replies is the server's onMessage dispatch (http/server/HttpHandler.cpp:
// 174-200) over the piece table of hvws_messages: each segment's first closing
// piece (one atomic min per closing piece -- closes are rare), then flag, scan
// and scatter into a dense table of hvws_tx_msg the send reads in place.
// hvws_replies_checked adds hvws_check's fail_rec as a second per-segment limit
// (rep_load::fail; null for hvws_replies, whose branches are then the old ones).
//
// Traffic: 24 B read + 32 B of scan state per message, ~37 B written per frame;
// per piece 40 B read twice and 32 B written per reply.
#include "hvws_dev.h"

namespace hvws {

namespace {

// ---------------------------------------------------------------- the send

struct snd3 {
    uint64_t frames, bytes, bad;
};
__device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
__device__ __forceinline__ snd3 scan_op(const snd3& a, const snd3& b) {
    return snd3{sat_add(a.frames, b.frames), sat_add(a.bytes, b.bytes), sat_add(a.bad, b.bad)};
}

// hvws_frag_key of include/hvws.h
constexpr __host__ __device__ uint32_t frag_key(uint32_t k, uint32_t j) {
    if (j == 0) return k;
    uint32_t x = k + j * 0x9E3779B9u;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
static_assert(frag_key(0x12345678u, 1) == 0x047660EAu && frag_key(0x12345678u, 2) == 0x6072B3DCu &&
                  frag_key(0, 1) == 0x92CA2F0Eu && frag_key(0xFFFFFFFFu, 0xFFFFFFFFu) == 0x3B66B2AAu,
              "frag_key: the known answers of include/hvws.h");

// What message i adds to the scan.  Messages at or beyond the effective count
// (min(*n_dev, n); n_dev may be null) add the identity.
struct send_load {
    const dtxmsg* msgs;
    const uint64_t* n_dev;
    uint64_t n, plen, F;
    uint32_t masked;
    __device__ __forceinline__ uint64_t count() const {
        if (!n_dev) return n;
        const uint64_t d = *n_dev;
        return d < n ? d : n;
    }
    __device__ __forceinline__ snd3 operator()(uint64_t i) const {
        if (i >= count()) return snd3{};
        const dtxmsg m = msgs[i];
        if (m.off > plen || m.len > plen - m.off || (m.flags & ~0x1Fu)) return snd3{0, 0, 1};
        uint64_t fr, bytes;
        send_wire(m.len, F, masked, fr, bytes);   // hvws_dev.h
        return snd3{fr, bytes, 0};
    }
};

// meta[0..3] = frames, bytes, bad messages, effective count; meta[4] += the
// messages breaking the uniform layout (more than one frame, a length other
// than message 0's, a payload step other than message 1's or a negative one);
// meta[5..7] = off[0], off[1] - off[0], len[0].  first[i] = message i's first
// frame (count + 1 entries), msg_off likewise in output bytes (optional).
__global__ __launch_bounds__(256) void k_send_msgs(send_load in, const snd3* __restrict__ ex,
                                                   const snd3* __restrict__ total, uint64_t* __restrict__ first,
                                                   uint64_t* __restrict__ msg_off,
                                                   unsigned long long* __restrict__ meta) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t cnt = in.count();
    const snd3 t = *total;
    bool nu = false;
    if (i == 0) {
        meta[0] = t.frames;
        meta[1] = t.bytes;
        meta[2] = t.bad;
        meta[3] = cnt;
        first[cnt] = t.frames;
        if (msg_off) msg_off[cnt] = t.bytes;
        meta[5] = cnt ? in.msgs[0].off : 0;
        meta[6] = cnt > 1 ? in.msgs[1].off - in.msgs[0].off : 0;
        meta[7] = cnt ? in.msgs[0].len : 0;
    }
    if (i < cnt) {
        const snd3 e = ex[i];
        first[i] = e.frames;
        if (msg_off) msg_off[i] = e.bytes;
        const dtxmsg m = in.msgs[i];
        nu = m.len > in.F;
        if (i) {
            const uint64_t p0 = in.msgs[0].off, p1 = in.msgs[1].off, pp = in.msgs[i - 1].off;
            nu = nu || m.len != in.msgs[0].len || p1 < p0 || m.off < pp || m.off - pp != p1 - p0;
        }
    }
    const uint64_t mu = __ballot(nu);
    if ((threadIdx.x & 63) == 0 && mu) atomicAdd(meta + 4, (unsigned long long)__popcll(mu));
}

// One thread per frame: the rows k_build reads.
__global__ __launch_bounds__(256) void k_send_expand(const dtxmsg* __restrict__ msgs, const snd3* __restrict__ ex,
                                                     const uint64_t* __restrict__ first,
                                                     const unsigned long long* __restrict__ meta, uint64_t nframes,
                                                     uint64_t F, uint32_t masked, uint64_t* __restrict__ pay_off,
                                                     uint64_t* __restrict__ len, uint8_t* __restrict__ flags,
                                                     uint32_t* __restrict__ mask, uint64_t* __restrict__ out_off,
                                                     uint64_t* __restrict__ size) {
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t cnt = meta[3];
    if (f >= nframes || cnt == 0) return;
    // the last message whose first frame is <= f (every message has a frame)
    uint64_t lo = 0, hi = cnt;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (first[mid] <= f) lo = mid;
        else hi = mid;
    }
    const dtxmsg m = msgs[lo];
    const uint64_t f0 = first[lo], nfr = first[lo + 1] - f0, j = f - f0;
    uint64_t ln = m.len;
    uint32_t fl = m.flags & 0x1Fu;
    if (nfr > 1) {   // OPCODE, CONTINUE ..., CONTINUE + FIN (WebSocketChannel.cpp:31-44)
        ln = j + 1 < nfr ? F : m.len - (nfr - 1) * F;
        fl = (j == 0 ? m.flags & F_OPMASK : 0u) | (j + 1 == nfr ? F_FIN : 0u);
    }
    pay_off[f] = m.off + j * F;
    len[f] = ln;
    flags[f] = (uint8_t)(fl | (masked ? F_MASK : 0u));
    mask[f] = masked ? frag_key(m.key, (uint32_t)j) : 0u;
    out_off[f] = ex[lo].bytes + j * (send_hdr(F, masked) + F);
    size[f] = send_hdr(ln, masked) + ln;
}

// -------------------------------------------------------------- the replies

// The reply opcode of a piece under `policy` (0: none): only complete
// messages are dispatched (HttpHandler.cpp:174-200).
__device__ __forceinline__ uint32_t reply_op(uint32_t info, uint32_t policy) {
    if (!(info & M_END)) return 0;
    const uint32_t op = info & F_OPMASK;
    if (op == 9 && (policy & R_PONG)) return 10;
    if (op == 8 && (policy & R_CLOSE)) return 8;
    if ((op == 1 || op == 2) && (policy & R_ECHO)) return op;
    return 0;
}

// limit[s]: pieces of segment s at or beyond it send nothing (~0: no limit).
// by_rec (after hvws_messages_rfc, whose pieces are not in stream order: data
// pieces before control pieces): the limit is 1 + the rec of the selected CLOSE
// piece with the smallest rec, and a piece sends when its rec lies below that
// record or when it is that CLOSE itself.
__global__ __launch_bounds__(256) void k_rep_init(const uint8_t* __restrict__ closed_in, uint32_t nseg,
                                                  unsigned long long* __restrict__ limit) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nseg) limit[s] = closed_in && closed_in[s] ? 0ull : ~0ull;
}

__device__ __forceinline__ uint64_t rep_pieces(const uint64_t* meta, uint64_t cap) { return meta[2] < cap ? meta[2] : cap; }

__global__ __launch_bounds__(256) void k_rep_close(const dmsg* __restrict__ msgs, const uint64_t* __restrict__ mg_meta,
                                                   uint64_t cap, uint32_t policy, uint32_t by_rec,
                                                   unsigned long long* __restrict__ limit) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= rep_pieces(mg_meta, cap)) return;
    const dmsg m = msgs[p];
    // an END piece has a record: rec + 1 does not wrap
    if (reply_op(m.info, policy) == 8) atomicMin(&limit[m.seg], (unsigned long long)((by_rec ? m.rec : p) + 1));
}

// 1 for a piece that is answered on the device
struct rep_load {
    const dmsg* msgs;
    const uint64_t* mg_meta;
    uint64_t cap;
    uint32_t policy;
    const unsigned long long* limit;
    uint32_t by_rec;
    // hvws_replies_checked: hvws_check's fail_rec per segment, a second limit by
    // rec (a CLOSE exactly there is itself malformed: not echoed); else null
    const unsigned long long* fail;
    __device__ __forceinline__ uint64_t operator()(uint64_t p) const {
        if (p >= rep_pieces(mg_meta, cap)) return 0;
        const dmsg m = msgs[p];
        const uint32_t op = reply_op(m.info, policy);
        if (!op || m.total != m.len) return 0;
        if (fail && m.rec >= fail[m.seg]) return 0;
        const unsigned long long lim = limit[m.seg];
        if (by_rec) return m.rec + 1 < lim || (m.rec + 1 == lim && op == 8) ? 1u : 0u;
        return p < lim ? 1u : 0u;
    }
};

__global__ __launch_bounds__(256) void k_rep_scatter(rep_load in, const uint64_t* __restrict__ ex,
                                                     dtxmsg* __restrict__ out, uint64_t* __restrict__ piece) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!in(p)) return;
    const dmsg m = in.msgs[p];
    const uint64_t i = ex[p];
    out[i] = dtxmsg{m.off, m.len, reply_op(m.info, in.policy) | F_FIN, 0u};
    piece[i] = p;
}

__global__ __launch_bounds__(256) void k_rep_segs(rep_load in, const uint64_t* __restrict__ ex,
                                                  const uint64_t* __restrict__ total,
                                                  const uint64_t* __restrict__ seg_first,
                                                  const uint64_t* __restrict__ seg_count, uint32_t nseg,
                                                  uint64_t* __restrict__ rep_first, uint64_t* __restrict__ rep_count,
                                                  uint8_t* __restrict__ flags) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const uint64_t np = rep_pieces(in.mg_meta, in.cap);
    uint64_t p0 = seg_first[s], cnt = seg_count[s];
    if (p0 > np) p0 = np;
    if (cnt > np - p0) cnt = np - p0;
    const uint64_t a = p0 < np ? ex[p0] : *total, b = p0 + cnt < np ? ex[p0 + cnt] : *total;
    rep_first[s] = a;
    rep_count[s] = b - a;
    const unsigned long long lim = in.limit[s];
    uint32_t fl = lim != ~0ull ? RF_CLOSED : 0u;
    if (in.fail && in.fail[s] != ~0ull) fl |= RF_FAILED | RF_CLOSED;
    if (cnt && lim > p0 && !in.by_rec) {   // only a segment's first piece can complete an earlier batch's message
        const dmsg m = in.msgs[p0];
        if (reply_op(m.info, in.policy) && m.total != m.len) fl |= RF_DEFERRED;
    }
    flags[s] = (uint8_t)fl;
}

}  // namespace

uint64_t send_scratch_bytes(uint64_t n) { return (n + 16 + scan_tmp_words(n)) * sizeof(snd3); }

hipError_t launch_send_table(const dtxmsg* msgs, uint64_t n, const uint64_t* n_dev, uint64_t plen, uint64_t F,
                             int masked, void* scratch, uint64_t* first, uint64_t* msg_off, uint64_t* meta,
                             hipStream_t st) {
    snd3* ex = reinterpret_cast<snd3*>(scratch);
    snd3* total = ex + n;   // one value; 16 are set aside
    snd3* tmp = ex + n + 16;
    const send_load in{msgs, n_dev, n, plen, F, masked ? 1u : 0u};
    hipError_t e = launch_scan_of(in, ex, n, tmp, total, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_send_msgs, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, in, ex, total, first, msg_off,
                       reinterpret_cast<unsigned long long*>(meta));
    return hipGetLastError();
}

hipError_t launch_send_expand(const dtxmsg* msgs, const void* scratch, const uint64_t* first, const uint64_t* meta,
                              uint64_t nframes, uint64_t F, int masked, uint64_t* pay_off, uint64_t* len,
                              uint8_t* flags, uint32_t* mask, uint64_t* out_off, uint64_t* size, hipStream_t st) {
    if (nframes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_send_expand, dim3((uint32_t)((nframes + 255) / 256)), dim3(256), 0, st, msgs,
                       reinterpret_cast<const snd3*>(scratch), first,
                       reinterpret_cast<const unsigned long long*>(meta), nframes, F, masked ? 1u : 0u, pay_off, len,
                       flags, mask, out_off, size);
    return hipGetLastError();
}

uint64_t rep_scratch_words(uint64_t cap) { return cap + 16 + scan_tmp_words(cap); }

hipError_t launch_replies(const dmsg* msgs, const uint64_t* mg_meta, uint64_t cap, const uint64_t* seg_first,
                          const uint64_t* seg_count, uint32_t nseg, uint32_t policy, const uint8_t* closed_in,
                          uint64_t* limit, uint64_t* scratch, dtxmsg* out, uint64_t* piece, uint64_t* rep_first,
                          uint64_t* rep_count, uint8_t* flags, bool by_rec, hipStream_t st, const uint64_t* fail) {
    unsigned long long* lim = reinterpret_cast<unsigned long long*>(limit);
    uint64_t* ex = scratch;
    uint64_t* total = ex + cap;   // the reply count: the send's d_n
    uint64_t* tmp = ex + cap + 16;
    const uint32_t sb = (nseg + 255) / 256, pb = (uint32_t)((cap + 255) / 256);
    if (sb) hipLaunchKernelGGL(k_rep_init, dim3(sb), dim3(256), 0, st, closed_in, nseg, lim);
    if (pb) hipLaunchKernelGGL(k_rep_close, dim3(pb), dim3(256), 0, st, msgs, mg_meta, cap, policy, by_rec ? 1u : 0u,
                               lim);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const rep_load in{msgs, mg_meta, cap, policy, lim, by_rec ? 1u : 0u,
                      reinterpret_cast<const unsigned long long*>(fail)};
    e = launch_scan_of(in, ex, cap, tmp, total, st);
    if (e != hipSuccess) return e;
    if (pb) hipLaunchKernelGGL(k_rep_scatter, dim3(pb), dim3(256), 0, st, in, ex, out, piece);
    if (sb)
        hipLaunchKernelGGL(k_rep_segs, dim3(sb), dim3(256), 0, st, in, ex, total, seg_first, seg_count, nseg, rep_first,
                           rep_count, flags);
    return hipGetLastError();
}

}  // namespace hvws
