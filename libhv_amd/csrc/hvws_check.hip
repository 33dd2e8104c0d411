// hvws_check.hip -- the kernels of hvws_check (include/hvws.h has the contract):
// which connections of a batch must be failed (RFC 6455 sec. 7.1.7), at which
// record and with which close code, from the tables the earlier passes left on
// the device.
//
// The pass reads the frame table (info, length), the piece table of
// hvws_messages_rfc, the verdicts of hvws_utf8 and, for Close frames only, at
// most 125 bytes of that message call's output each.  It writes tables of its
// own and nothing another pass reads.
//
//   the sequence scan  RFC 6455 sec. 5.4 per connection is a walk over its data
//                      headers: CONTINUE needs an open message, TEXT / BINARY
//                      need none, and every such header then SETS the open bit
//                      to "FIN clear".  Every relevant record overwrites the
//                      state, so the state before record r is that of the last
//                      writer before r: one device-wide exclusive scan (the scan
//                      of hvws_dev.h) over all records of the batch whose value
//                      is (writer's record index + 1) << 1 | open and whose
//                      operator keeps the later non-zero value.  The reset at a
//                      connection's start needs no flag in the scan: a writer
//                      with an index below the connection's first record belongs
//                      to another connection, and the state is then the one
//                      carried in.  One connection of a million records spreads
//                      over the device exactly as a million connections of one.
//   k_chk_find         one thread per record and per piece: the violation
//                      classes found there (kept in one byte each) and an
//                      atomicMin of the record index into the connection's
//                      fail_rec.  A Close body is read by the piece's lane in
//                      aligned 16-byte loads that stay inside [off, off + len)
//                      rounded outwards to 16 bytes and clipped to the buffer.
//   k_chk_why          the same threads, once the minima are final: the classes
//                      found at exactly fail_rec are ORed into why.
//   k_chk_final        one thread per connection: close code, state word out.
//
// Traffic: 4 B of info per record twice, 8 B of scan state written and read, 8 B
// of length for data headers when a size limit is set, 40 B per piece, one
// byte of violation classes per record and piece written and read.
#include "hvws_dev.h"

namespace hvws {

namespace {

constexpr unsigned long long CHK_NONE = ~0ull;

// (writer's record index + 1) << 1 | open; 0: no writer yet (the identity)
struct lastw {
    uint64_t v;
};
__device__ __forceinline__ lastw scan_op(const lastw& a, const lastw& b) { return b.v ? b : a; }

__device__ __forceinline__ uint64_t chk_records(const uint64_t* nfr_p, uint64_t cap) {
    const uint64_t n = *nfr_p;
    return n < cap ? n : cap;
}

// a record that takes part in the sequence rule: a completed data header of
// opcode 0, 1 or 2 (3 .. 7 are the header class's)
__device__ __forceinline__ bool seq_record(uint32_t inf) { return (inf & I_HDR) && (inf & F_OPMASK) <= 2u; }

struct seq_load {
    const uint32_t* info;
    const uint64_t* nfr_p;
    uint64_t cap;
    __device__ __forceinline__ lastw operator()(uint64_t r) const {
        if (r >= chk_records(nfr_p, cap)) return lastw{};
        const uint32_t inf = info[r];
        if (!seq_record(inf)) return lastw{};
        return lastw{((r + 1) << 1) | ((inf & F_FIN) ? 0u : 1u)};
    }
};

// What every kernel of the pass needs to place a record in its connection.
struct chk_segs {
    const uint64_t* bases;
    const uint64_t* nfr_p;
    uint64_t cap;
    uint32_t nseg;
    const uint32_t* state_in;   // nullptr: all fresh
    __device__ __forceinline__ uint64_t records() const { return chk_records(nfr_p, cap); }
    __device__ __forceinline__ uint64_t first(uint32_t s, uint64_t n) const { return bases[s] < n ? bases[s] : n; }
    __device__ __forceinline__ uint32_t word(uint32_t s) const { return state_in ? state_in[s] : 0u; }
    // the last connection whose first record is <= r (connection 0's is 0); nseg > 0
    __device__ __forceinline__ uint32_t seg_of(uint64_t r, uint64_t n) const {
        uint32_t lo = 0, hi = nseg;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (first(mid, n) > r) hi = mid;
            else lo = mid + 1;
        }
        return lo - 1u;
    }
    // the open bit a scan value stands for in connection s
    __device__ __forceinline__ uint32_t open_of(lastw w, uint32_t s, uint64_t n) const {
        if (w.v && (w.v >> 1) - 1 >= first(s, n)) return (uint32_t)(w.v & 1u);
        return word(s) & CK_OPEN;
    }
};

// hvws_utf8's machine (include/hvws.h): the state after byte b in state s
__device__ __forceinline__ uint32_t u8_step(uint32_t s, uint32_t b) {
    if (s == 0) {
        if (b < 0x80u) return 0;
        if (b >= 0xC2u && b <= 0xDFu) return 1;
        if (b == 0xE0u) return 3;
        if (b == 0xEDu) return 4;
        if (b >= 0xE1u && b <= 0xEFu) return 2;
        if (b == 0xF0u) return 5;
        if (b >= 0xF1u && b <= 0xF3u) return 6;
        if (b == 0xF4u) return 7;
        return U8_REJECT;
    }
    if (s > 7) return U8_REJECT;
    const uint32_t lo = s == 3 ? 0xA0u : (s == 5 ? 0x90u : 0x80u);
    const uint32_t hi = s == 4 ? 0x9Fu : (s == 7 ? 0x8Fu : 0xBFu);
    if (b < lo || b > hi) return U8_REJECT;
    return s == 1 ? 0u : (s <= 4 ? 1u : 2u);
}

__device__ __forceinline__ bool close_code_ok(uint32_t code) {
    return (code >= 1000 && code <= 1003) || (code >= 1007 && code <= 1011) || (code >= 3000 && code <= 4999);
}

// The classes a Close body of 2 .. 125 bytes at out[off, off + len) violates.
// Loads are 16 bytes at 16-byte aligned addresses from off & ~15 up to the
// block holding the body's last byte; a block that would cross out_len is read
// byte by byte below it.  Nothing outside [0, out_len) is touched.
__device__ __forceinline__ uint32_t close_body_bits(const uint8_t* __restrict__ out, uint64_t out_len, uint64_t off,
                                                    uint64_t len) {
    const uint64_t end = off + len;
    uint32_t st = U8_ACCEPT, code = 0;
    for (uint64_t a = off & ~15ull; a < end; a += 16) {
        u32x4 v{0u, 0u, 0u, 0u};
        if (a + 16 <= out_len) {
            v = *reinterpret_cast<const u32x4*>(out + a);
        } else {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (a + b < out_len) w[b >> 2] |= (uint32_t)out[a + b] << (8 * (b & 3));
            v = u32x4{w[0], w[1], w[2], w[3]};
        }
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const uint64_t q = a + b;
            const uint32_t w = b < 4 ? v.x : (b < 8 ? v.y : (b < 12 ? v.z : v.w));
            const uint32_t byte = (w >> (8 * (b & 3))) & 0xFFu;
            if (q < off || q >= end) continue;
            const uint64_t k = q - off;
            if (k == 0) code = byte << 8;
            else if (k == 1) code |= byte;
            else st = u8_step(st, byte);
        }
    }
    return (close_code_ok(code) ? 0u : CK_CLOSE_BODY) | (len > 2 && st != U8_ACCEPT ? CK_CLOSE_UTF8 : 0u);
}

__global__ __launch_bounds__(256) void k_chk_init(chk_segs sg, const uint64_t* __restrict__ u8_bad,
                                                  unsigned long long* __restrict__ fail, uint32_t* __restrict__ why) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= sg.nseg) return;
    unsigned long long f = CHK_NONE;
    if (sg.word(s) & CK_FAILED) f = sg.first(s, sg.records());
    else if (u8_bad) f = u8_bad[s];
    fail[s] = f;
    why[s] = 0u;
}

// The classes record r violates; s is its connection.
__device__ __forceinline__ uint32_t record_bits(const chk_segs& sg, uint64_t r, uint64_t n, uint32_t s, uint32_t inf,
                                                const lastw* __restrict__ ex, const uint64_t* __restrict__ length,
                                                uint32_t classes, uint64_t max_message) {
    uint32_t bits = 0;
    if ((classes & CK_HEADER) && (inf & I_INVALID)) bits |= CK_HEADER;
    if ((classes & CK_SEQUENCE) && seq_record(inf)) {
        const uint32_t open = sg.open_of(ex[r], s, n);
        if ((inf & F_OPMASK) == 0u ? !open : open) bits |= CK_SEQUENCE;
    }
    if ((classes & CK_SIZE) && max_message && (inf & I_HDR) && (inf & F_OPMASK) < 8u && length[r] > max_message)
        bits |= CK_SIZE;
    return bits;
}

// The classes piece m violates.
__device__ __forceinline__ uint32_t piece_bits(const dmsg& m, const uint8_t* __restrict__ out, uint64_t out_len,
                                               uint32_t classes, uint64_t max_message) {
    if (m.info & M_CTL) {
        if (!(m.info & M_END) || (m.info & F_OPMASK) != 8u || !(classes & (CK_CLOSE_BODY | CK_CLOSE_UTF8))) return 0;
        if (m.len == 0) return 0;
        if (m.len == 1 || m.len > 125) return classes & CK_CLOSE_BODY;   // judged from len alone, never read
        return close_body_bits(out, out_len, m.off, m.len) & classes;
    }
    return (classes & CK_SIZE) && max_message && m.len > max_message ? CK_SIZE : 0u;
}

// Thread i: record i and piece i.  viol[0 .. cap): the records' classes,
// viol[cap .. cap + pcap): the pieces'.  A connection carried in as failed
// finds nothing new.
__global__ __launch_bounds__(256) void k_chk_find(chk_segs sg, const uint32_t* __restrict__ info,
                                                  const uint64_t* __restrict__ length, const lastw* __restrict__ ex,
                                                  const dmsg* __restrict__ msgs, const uint64_t* __restrict__ mg_meta,
                                                  uint64_t pcap, const uint8_t* __restrict__ out, uint64_t out_len,
                                                  uint32_t classes, uint64_t max_message,
                                                  uint8_t* __restrict__ viol, unsigned long long* __restrict__ fail) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = sg.records();
    uint32_t rbits = 0, rseg = ~0u;
    if (i < n) {
        const uint32_t inf = info[i];
        // only a record that can violate something looks for its connection
        if ((inf & I_INVALID) || (inf & I_HDR)) {
            const uint32_t s = sg.seg_of(i, n);
            if (!(sg.word(s) & CK_FAILED)) {
                rbits = record_bits(sg, i, n, s, inf, ex, length, classes, max_message);
                if (rbits) rseg = s;
            }
        }
        viol[i] = (uint8_t)rbits;
    }
    // A violating record whose left neighbour in the wave violates in the same
    // connection cannot be the minimum: a batch in which every record violates
    // sends one atomic per wave and connection, not one per record.
    const uint32_t left = __shfl_up(rseg, 1);
    if (rbits && !((threadIdx.x & 63u) && left == rseg)) atomicMin(&fail[rseg], (unsigned long long)i);
    const uint64_t np = mg_meta[2] < pcap ? mg_meta[2] : pcap;
    if (i < np) {
        const dmsg m = msgs[i];
        uint32_t bits = 0;
        if (m.seg < sg.nseg && !(sg.word(m.seg) & CK_FAILED)) {
            bits = piece_bits(m, out, out_len, classes, max_message);
            if (bits) atomicMin(&fail[m.seg], (unsigned long long)(m.rec == ~0ull ? sg.first(m.seg, n) : m.rec));
        }
        viol[sg.cap + i] = (uint8_t)bits;
    }
}

__global__ __launch_bounds__(256) void k_chk_why(chk_segs sg, const dmsg* __restrict__ msgs,
                                                 const uint64_t* __restrict__ mg_meta, uint64_t pcap,
                                                 const uint8_t* __restrict__ viol,
                                                 const unsigned long long* __restrict__ fail,
                                                 uint32_t* __restrict__ why) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = sg.records();
    if (i < n) {
        const uint32_t bits = viol[i];
        if (bits) {
            const uint32_t s = sg.seg_of(i, n);
            if (fail[s] == i) atomicOr(&why[s], bits);
        }
    }
    const uint64_t np = mg_meta[2] < pcap ? mg_meta[2] : pcap;
    if (i < np) {
        const uint32_t bits = viol[sg.cap + i];
        if (bits) {
            const dmsg m = msgs[i];
            const uint64_t rec = m.rec == ~0ull ? sg.first(m.seg, n) : m.rec;
            if (fail[m.seg] == rec) atomicOr(&why[m.seg], bits);
        }
    }
}

__device__ __forceinline__ uint32_t close_code_of(uint32_t why) {
    if (why & (CK_HEADER | CK_SEQUENCE | CK_CLOSE_BODY)) return 1002u;
    if (why & (CK_CLOSE_UTF8 | CK_TEXT_UTF8)) return 1007u;
    if (why & CK_SIZE) return 1009u;
    return 0u;
}

__global__ __launch_bounds__(256) void k_chk_final(chk_segs sg, const lastw* __restrict__ ex,
                                                   const lastw* __restrict__ total,
                                                   const uint64_t* __restrict__ u8_bad,
                                                   const unsigned long long* __restrict__ fail,
                                                   uint32_t* __restrict__ why, uint16_t* __restrict__ code,
                                                   uint32_t* __restrict__ state_out) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= sg.nseg) return;
    const uint64_t n = sg.records();
    const unsigned long long f = fail[s];
    uint32_t w = why[s];
    if (u8_bad && f != CHK_NONE && !(sg.word(s) & CK_FAILED) && u8_bad[s] == f) w |= CK_TEXT_UTF8;
    why[s] = w;
    code[s] = (uint16_t)close_code_of(w);
    if (f != CHK_NONE) {
        state_out[s] = CK_FAILED;
        return;
    }
    const uint64_t re = s + 1 < sg.nseg ? sg.first(s + 1, n) : n;
    state_out[s] = sg.open_of(re < n ? ex[re] : *total, s, n);
}

}  // namespace

uint64_t check_scratch_bytes(uint64_t cap) { return (cap + 16 + scan_tmp_words(cap)) * sizeof(lastw); }

hipError_t launch_check(const uint32_t* info, const uint64_t* length, const uint64_t* nfr_dev, uint64_t cap,
                        const uint64_t* bases, uint32_t nseg, const dmsg* msgs, const uint64_t* mg_meta, uint64_t pcap,
                        const uint8_t* out, uint64_t out_len, const uint64_t* u8_bad, uint32_t classes,
                        uint64_t max_message, const uint32_t* state_in, void* scratch, uint8_t* viol, uint32_t* state_out,
                        uint64_t* fail, uint32_t* why, uint16_t* code, hipStream_t st) {
    if (nseg == 0) return hipSuccess;
    lastw* ex = reinterpret_cast<lastw*>(scratch);
    lastw* total = ex + cap;   // one value; 16 are set aside
    lastw* tmp = ex + cap + 16;
    unsigned long long* fl = reinterpret_cast<unsigned long long*>(fail);
    const chk_segs sg{bases, nfr_dev, cap, nseg, state_in};
    const uint32_t sb = (nseg + 255) / 256;
    const uint64_t ne = cap > pcap ? cap : pcap;
    const uint32_t eb = (uint32_t)((ne + 255) / 256);
    hipLaunchKernelGGL(k_chk_init, dim3(sb), dim3(256), 0, st, sg, (classes & CK_TEXT_UTF8) ? u8_bad : nullptr, fl, why);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan_of(seq_load{info, nfr_dev, cap}, ex, cap, tmp, total, st);
    if (e != hipSuccess) return e;
    if (eb) {
        hipLaunchKernelGGL(k_chk_find, dim3(eb), dim3(256), 0, st, sg, info, length, ex, msgs, mg_meta, pcap, out, out_len,
                           classes, max_message, viol, fl);
        hipLaunchKernelGGL(k_chk_why, dim3(eb), dim3(256), 0, st, sg, msgs, mg_meta, pcap, viol, fl, why);
    }
    hipLaunchKernelGGL(k_chk_final, dim3(sb), dim3(256), 0, st, sg, ex, total,
                       (classes & CK_TEXT_UTF8) ? u8_bad : nullptr, fl, why, code, state_out);
    return hipGetLastError();
}

}  // namespace hvws
