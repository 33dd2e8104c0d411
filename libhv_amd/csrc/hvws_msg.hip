// hvws_msg.hip -- message reassembly on the device (the reference's
// WebSocketParser::FeedRecvData, http/WebSocketParser.cpp:8-75, over the frame
// table of the last scan).  include/hvws.h has the contract: the message rule
// over frame records, the output layout, pieces, the carried state.
//
// The operation is a stream compaction driven by the frame table.  Two parts:
//
//   the table pass   one device-wide scan over the records (the scan of
//                    hvws_dev.h, shared with the transmit side) carries, per
//                    record r, three quantities at once:
//                      bytes  sum of pay_len before r         -> out_off[r]
//                      close  piece-closing records before r  -> r's piece
//                      latch  1 + the last record at or before r whose header
//                             latches an opcode (a running maximum; 0 = none;
//                             below the segment's base = the state carried in)
//                    A record closes a piece when a FIN frame ends at it or
//                    when it is its segment's last.  Work is spread by records:
//                    one connection with a million records takes as many
//                    workgroups as a million connections with one each.
//                    k_msg_records then writes out_off and each piece's last
//                    record, k_msg_pieces one hvws_msg per piece, k_msg_segs
//                    each segment's first / count and the state to carry on.
//   k_msg_gather     the only pass over the payload bytes.  Tiled over the
//                    OUTPUT (4 or 16 KiB per workgroup, 16-byte aligned
//                    stores); a tile finds its records from a tile index over
//                    (out_off, pay_len) -- the unmask's index kernels, run on
//                    output offsets.  A tile inside one record streams: two
//                    16-byte loads per chunk at the record's misalignment,
//                    funnel-shifted, XORed with the key word rotated to the
//                    chunk's phase.  Other tiles stage their records in LDS and
//                    build chunk by chunk; a chunk holding record boundaries
//                    walks its pieces (records of 0 bytes contribute nothing).
//
// Traffic: payload read + payload written + ~100 bytes per record of tables.
// No source read leaves [rx, rx + rx_len); no byte at or beyond
// min(payload total, out_cap) is written.
//
// The joined form (hvws_messages_joined) runs the same two parts over ROWS:
// each segment's carried span -- the bytes of its open message, lying in the
// previous call's output -- is a row ahead of the segment's records, so row
// b(s) = min(bases[s], records) + s is segment s's carried row and record r of
// segment s is row r + s + 1.  k_join_rows writes the row table once (length,
// source with a buffer selector, key, info with the piece-closing bit); the
// scan, the three table kernels, the tile index and the gather then take rows
// where the plain form takes records, and the work stays spread by rows.
//
// The RFC form (hvws_messages_rfc) is the joined form over two virtual
// connections per connection, the data records and the control records: one
// more scan ranks every record within its class, k_rfc_rows scatters the rows
// into output order (per connection: data carried row, data records, control
// carried row, control records), and everything from the scan on runs over
// those rows as it does over the joined form's.
#include <stdlib.h>

#include "hvws_dev.h"

namespace hvws {

namespace {

struct msg3 {
    uint64_t bytes, close, latch;
};
__device__ __forceinline__ msg3 scan_op(const msg3& a, const msg3& b) {
    return msg3{a.bytes + b.bytes, a.close + b.close, a.latch > b.latch ? a.latch : b.latch};
}

// first s in [0, nseg) with bases[s] > r (nseg if none): s - 1 is r's segment
__device__ __forceinline__ uint32_t seg_after(const uint64_t* __restrict__ bases, uint32_t nseg, uint64_t r) {
    uint32_t lo = 0, hi = nseg;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (bases[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// What record r adds to the scan.  Records at or beyond the batch's count
// (on the device, clamped to the table's capacity) add the identity.
struct msg_load {
    const uint64_t* pay_len;
    const uint32_t* info;
    const uint64_t* nfr_p;
    uint64_t cap;
    const uint64_t* bases;
    uint32_t nseg;
    static constexpr bool JOINED = false;
    static constexpr bool RFC = false;
    __device__ __forceinline__ uint64_t nrec() const { return *nfr_p < cap ? *nfr_p : cap; }
    __device__ __forceinline__ static bool fin_end(uint32_t inf) { return (inf & I_END) && (inf & F_FIN); }
    __device__ __forceinline__ uint64_t len(uint64_t r) const { return pay_len[r]; }
    __device__ __forceinline__ uint32_t inf(uint64_t r) const { return info[r]; }
    __device__ __forceinline__ uint32_t seg_of(uint64_t r) const { return seg_after(bases, nseg, r) - 1u; }
    __device__ __forceinline__ uint64_t base(uint32_t s) const { return bases[s]; }
    __device__ __forceinline__ msg3 operator()(uint64_t r) const {
        const uint64_t n = nrec();
        if (r >= n) return msg3{};
        const uint32_t inf = info[r];
        bool closes = fin_end(inf) || r + 1 == n;
        if (!closes) {   // the segment's last record: another segment begins at r + 1
            const uint32_t s = seg_after(bases, nseg, r);
            closes = s < nseg && bases[s] == r + 1;
        }
        const uint64_t latch = (inf & I_HDR) && (inf & F_OPMASK) ? r + 1 : 0;
        return msg3{pay_len[r], closes ? 1u : 0u, latch};
    }
};

// ---- the joined form's rows
constexpr uint64_t ROW_PREV = 1ull << 63;   // a row's source word: an offset into prev, not rx
constexpr uint32_t ROW_CLOSE = 1u << 31;    // a row's info: it closes a piece (the frame info ends below bit 24)

// Rows where msg_load has records.  nrec() counts rows; a row's info is its
// record's (0 for a carried row) with ROW_CLOSE worked out by k_join_rows.
struct row_load {
    const uint64_t* row_len;
    const uint32_t* row_info;
    const uint64_t* nfr_p;
    uint64_t cap;   // records
    const uint64_t* bases;
    uint32_t nseg;
    static constexpr bool JOINED = true;
    static constexpr bool RFC = false;
    __device__ __forceinline__ uint64_t records() const { return *nfr_p < cap ? *nfr_p : cap; }
    __device__ __forceinline__ uint64_t nrec() const { return records() + nseg; }
    __device__ __forceinline__ static bool fin_end(uint32_t inf) { return (inf & I_END) && (inf & F_FIN); }
    __device__ __forceinline__ uint64_t len(uint64_t i) const { return row_len[i]; }
    __device__ __forceinline__ uint32_t inf(uint64_t i) const { return row_info[i]; }
    // segment s's carried row (a table cut short by its capacity leaves later segments without records)
    __device__ __forceinline__ uint64_t base(uint32_t s) const {
        const uint64_t n = records(), b = bases[s];
        return (b < n ? b : n) + s;
    }
    // the last segment whose carried row is at or before row i (nseg > 0: row 0 is segment 0's)
    __device__ __forceinline__ uint32_t seg_of(uint64_t i) const {
        uint32_t lo = 0, hi = nseg;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (base(mid) > i) hi = mid;
            else lo = mid + 1;
        }
        return lo - 1u;
    }
    __device__ __forceinline__ msg3 operator()(uint64_t i) const {
        if (i >= nrec()) return msg3{};
        const uint32_t inf = row_info[i];
        const uint64_t latch = (inf & I_HDR) && (inf & F_OPMASK) ? i + 1 : 0;
        return msg3{row_len[i], inf & ROW_CLOSE ? 1u : 0u, latch};
    }
};

// The row table, one thread per row.  A carried row: P = state_in[s].pending
// bytes at prev_off[s] of prev, no key; it closes a piece only when the segment
// has no records and P > 0 (the piece without a record).  A record's row: the
// record's source, key and info; it closes a piece when a FIN frame ends at it
// or when it is its segment's last.
__global__ __launch_bounds__(256) void k_join_rows(row_load in, const uint64_t* __restrict__ pay_off,
                                                   const uint64_t* __restrict__ pay_len,
                                                   const uint32_t* __restrict__ info,
                                                   const uint32_t* __restrict__ keyrot, uint32_t masked,
                                                   const dmsg_state* __restrict__ state_in,
                                                   const uint64_t* __restrict__ prev_off,
                                                   uint64_t* __restrict__ row_len, uint64_t* __restrict__ row_src,
                                                   uint32_t* __restrict__ row_key, uint32_t* __restrict__ row_info) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t rows = in.nrec();
    if (i >= rows) return;
    const uint32_t s = in.seg_of(i);
    const uint64_t b = in.base(s);
    const bool last = i + 1 == (s + 1 < in.nseg ? in.base(s + 1) : rows);   // its segment's last row
    if (i == b) {
        const uint64_t P = state_in ? state_in[s].pending : 0;
        row_len[i] = P;
        row_src[i] = P ? ROW_PREV | prev_off[s] : 0;
        row_key[i] = 0;
        row_info[i] = last && P ? ROW_CLOSE : 0u;
    } else {
        const uint64_t r = i - s - 1;
        const uint32_t inf = info[r];
        row_len[i] = pay_len[r];
        row_src[i] = pay_off[r];
        row_key[i] = masked ? keyrot[r] : 0u;
        row_info[i] = inf | (row_load::fin_end(inf) || last ? ROW_CLOSE : 0u);
    }
}

// ---- the RFC form's rows (hvws_messages_rfc)
// Two virtual connections per connection: 2s takes the data records (opcode
// below 8), 2s + 1 the control records, each behind a carried row of its own.
// Connection s's rows begin at R(s) = min(bases[s], records) + 2s and lie in
// output order: the data carried row, the data records, the control carried
// row, the control records, then the records of neither class (a header still
// incomplete: no bytes, no latch, never a piece's last row), which ride at the
// end of 2s + 1 so that the batch has records + 2 nseg rows whatever it holds.
struct cls2 {
    uint64_t ctl, none;   // control records, records of neither class
};
__device__ __forceinline__ cls2 scan_op(const cls2& a, const cls2& b) { return cls2{a.ctl + b.ctl, a.none + b.none}; }

// 0: a data record, 1: a control record, 2: neither
__device__ __forceinline__ uint32_t rfc_class(uint32_t inf) {
    if (!(inf & (I_HDR | I_BODY | I_END))) return 2u;
    return (inf & F_OPMASK) >= 8u ? 1u : 0u;
}

struct cls_load {
    const uint32_t* info;
    const uint64_t* nfr_p;
    uint64_t cap;
    __device__ __forceinline__ cls2 operator()(uint64_t r) const {
        if (r >= (*nfr_p < cap ? *nfr_p : cap)) return cls2{};
        const uint32_t k = rfc_class(info[r]);
        return cls2{k == 1u ? 1u : 0u, k == 2u ? 1u : 0u};
    }
};

// The class scan's result for record r (block-relative values and block bases,
// as msg_scan below); records at or beyond cap read the total.
struct cls_scan {
    const cls2* ex;
    const cls2* base;   // nullptr: one block
    const cls2* total;
    uint64_t cap;
    __device__ __forceinline__ cls2 operator()(uint64_t r) const {
        if (r >= cap) return *total;
        const cls2 v = ex[r];
        return base ? scan_op(base[r / SCAN_B], v) : v;
    }
};

// row_load over the scattered rows.  nseg counts VIRTUAL connections; vbase[v]
// is v's carried row (strictly increasing) and row_rec a row's frame-table
// index.  A control frame is a message of its own: its END closes a piece with
// or without FIN (opcodes 8 .. 15 have bit 3).
struct rfc_load {
    const uint64_t* row_len;
    const uint32_t* row_info;
    const uint64_t* nfr_p;
    uint64_t cap;   // records
    const uint64_t* vbase;
    const uint64_t* row_rec;
    uint32_t nseg;
    static constexpr bool JOINED = true;
    static constexpr bool RFC = true;
    __device__ __forceinline__ uint64_t records() const { return *nfr_p < cap ? *nfr_p : cap; }
    __device__ __forceinline__ uint64_t nrec() const { return records() + nseg; }
    __device__ __forceinline__ static bool fin_end(uint32_t inf) { return (inf & I_END) && (inf & (F_FIN | 8u)); }
    __device__ __forceinline__ uint64_t len(uint64_t i) const { return row_len[i]; }
    __device__ __forceinline__ uint32_t inf(uint64_t i) const { return row_info[i]; }
    __device__ __forceinline__ uint64_t base(uint32_t v) const { return vbase[v]; }
    __device__ __forceinline__ uint64_t rec_of(uint64_t i) const { return row_rec[i]; }
    __device__ __forceinline__ uint32_t seg_of(uint64_t i) const {   // nseg > 0: row 0 is virtual connection 0's
        uint32_t lo = 0, hi = nseg;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (vbase[mid] > i) hi = mid;
            else lo = mid + 1;
        }
        return lo - 1u;
    }
    __device__ __forceinline__ msg3 operator()(uint64_t i) const {
        if (i >= nrec()) return msg3{};
        const uint32_t inf = row_info[i];
        const uint64_t latch = (inf & I_HDR) && (inf & F_OPMASK) ? i + 1 : 0;
        return msg3{row_len[i], inf & ROW_CLOSE ? 1u : 0u, latch};
    }
};

// The row table of the RFC form, one thread per row slot: slot R(s) writes
// connection s's data carried row (and vbase / vcnt of both virtual
// connections), slot R(s) + 1 its control carried row, slot R(s) + 2 + k the
// row of the connection's k-th record, each at its place in output order: the
// stable partition comes from cls, the exclusive scan of cls_load.  A carried
// row closes a piece only when its class has no records and bytes are pending;
// a record's row when its frame completes a message of its class or when it is
// its class's last in the connection.
__global__ __launch_bounds__(256) void k_rfc_rows(const uint64_t* __restrict__ nfr_p, uint64_t cap,
                                                  const uint64_t* __restrict__ bases, uint32_t nseg, cls_scan cls,
                                                  const uint64_t* __restrict__ pay_off,
                                                  const uint64_t* __restrict__ pay_len,
                                                  const uint32_t* __restrict__ info,
                                                  const uint32_t* __restrict__ keyrot, uint32_t masked,
                                                  const dmsg_state* __restrict__ vstate_in,
                                                  const uint64_t* __restrict__ voff, uint64_t* __restrict__ row_len,
                                                  uint64_t* __restrict__ row_src, uint32_t* __restrict__ row_key,
                                                  uint32_t* __restrict__ row_info, uint64_t* __restrict__ row_rec,
                                                  uint64_t* __restrict__ vbase, uint64_t* __restrict__ vcnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = *nfr_p < cap ? *nfr_p : cap;
    if (i >= n + 2ull * nseg) return;
    auto rbase = [&](uint32_t s) { return bases[s] < n ? bases[s] : n; };
    uint32_t lo = 0, hi = nseg;   // the last connection with R(s) <= i (R(0) = 0)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rbase(mid) + 2ull * mid > i) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t s = lo - 1u;
    const uint64_t rb = rbase(s), re = s + 1 < nseg ? rbase(s + 1) : n;
    const cls2 c0 = cls(rb), c1 = cls(re);
    const uint64_t nc = c1.ctl - c0.ctl, nn = c1.none - c0.none, nd = re - rb - nc - nn;
    const uint64_t R = rb + 2ull * s, j = i - R;
    if (j < 2) {   // a carried row
        const uint32_t v = 2u * s + (uint32_t)j;
        const uint64_t at_row = j ? R + 1 + nd : R, mine = j ? nc : nd;
        const uint64_t P = vstate_in ? vstate_in[v].pending : 0;
        row_len[at_row] = P;
        row_src[at_row] = P ? ROW_PREV | voff[v] : 0;
        row_key[at_row] = 0;
        row_info[at_row] = mine == 0 && P ? ROW_CLOSE : 0u;
        row_rec[at_row] = ~0ull;
        vbase[v] = at_row;
        vcnt[v] = mine;
        return;
    }
    const uint64_t r = rb + j - 2;
    const uint32_t inf = info[r];
    const uint32_t k = rfc_class(inf);
    const cls2 c = cls(r);
    const uint64_t kc = c.ctl - c0.ctl, kn = c.none - c0.none, kd = r - rb - kc - kn;
    if (k == 2u) {
        const uint64_t d = R + 2 + nd + nc + kn;
        row_len[d] = 0;
        row_src[d] = 0;
        row_key[d] = 0;
        row_info[d] = 0;
        row_rec[d] = r;
        return;
    }
    const uint64_t d = k ? R + 2 + nd + kc : R + 1 + kd;
    const bool last = k ? kc + 1 == nc : kd + 1 == nd;
    row_len[d] = pay_len[r];
    row_src[d] = pay_off[r];
    row_key[d] = masked ? keyrot[r] : 0u;
    row_info[d] = inf | (rfc_load::fin_end(inf) || last ? ROW_CLOSE : 0u);
    row_rec[d] = r;
}

// The scan's result for record r: its block-relative value and its block's base.
struct msg_scan {
    const msg3* ex;
    const msg3* base;   // nullptr: one block
    __device__ __forceinline__ msg3 operator()(uint64_t r) const {
        const msg3 v = ex[r];
        return base ? scan_op(base[r / SCAN_B], v) : v;
    }
};

// meta[0] = records, meta[1] = payload bytes, meta[2] = pieces.  Joined:
// meta[0] = rows, meta[1] includes the carried bytes, and each piece's last
// row goes to prow (msgs[].rec is then another number than the one read here).
template <typename LOAD>
__global__ __launch_bounds__(256) void k_msg_records(LOAD in, msg_scan sc, const msg3* __restrict__ total,
                                                     uint64_t* __restrict__ out_off, dmsg* __restrict__ msgs,
                                                     uint64_t* __restrict__ prow, uint64_t* __restrict__ meta) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = in.nrec();
    if (r == 0) {
        meta[0] = n;
        meta[1] = total->bytes;
        meta[2] = total->close;
    }
    if (r >= n) return;
    const msg3 e = sc(r);
    out_off[r] = e.bytes;
    if (in(r).close) {
        if constexpr (LOAD::JOINED) prow[e.close] = r;
        else msgs[e.close].rec = r;
    }
}

template <typename LOAD>
__global__ __launch_bounds__(256) void k_msg_pieces(LOAD in, msg_scan sc, const msg3* __restrict__ total,
                                                    const dmsg_state* __restrict__ state_in,
                                                    const uint64_t* __restrict__ prow, dmsg* __restrict__ msgs) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total->close) return;
    uint64_t r;
    if constexpr (LOAD::JOINED) r = prow[p];
    else r = msgs[p].rec;
    const msg3 e = sc(r);
    uint64_t off = 0, rp = 0;
    if (p) {
        if constexpr (LOAD::JOINED) rp = prow[p - 1];
        else rp = msgs[p - 1].rec;
        off = sc(rp).bytes + in.len(rp);
    }
    const uint32_t seg = in.seg_of(r);
    const uint64_t b = in.base(seg);   // joined: the carried row, below every latch of the segment
    const bool first = p == 0 || rp < b;   // the segment's first piece
    dmsg_state st = dmsg_state{0, 0, 0};
    if (state_in) st = state_in[seg];
    const uint32_t inf = in.inf(r);
    const msg3 own = in(r);
    const uint64_t latch = e.latch > own.latch ? e.latch : own.latch;
    uint32_t none = 8u;   // nothing latched (Q6)
    if constexpr (LOAD::RFC) none = seg & 1u ? 8u : 0u;   // ... which the RFC form's data class does not reproduce
    const uint32_t op = latch > b ? in.inf(latch - 1) & F_OPMASK : (st.opcode ? st.opcode : none);
    dmsg m;
    m.off = off;
    m.len = e.bytes + own.bytes - off;   // joined: the first piece's rows begin with the carried one
    if constexpr (LOAD::RFC) {
        m.total = m.len;
        m.rec = in.rec_of(r);   // ~0 for a carried row
    } else if constexpr (LOAD::JOINED) {
        m.total = m.len;
        m.rec = r == b ? ~0ull : r - seg - 1;   // a carried row closes the piece without a record
    } else {
        m.total = m.len + (first ? st.pending : 0);
        m.rec = r;
    }
    m.seg = seg;
    m.info = op | (LOAD::fin_end(inf) ? M_END : 0u) | (first && st.open ? M_CONT : 0u);
    if constexpr (LOAD::RFC) {   // seg counts virtual connections
        m.seg = seg >> 1;
        m.info |= seg & 1u ? M_CTL : 0u;
    }
    msgs[p] = m;
}

__global__ __launch_bounds__(256) void k_msg_segs(msg_load in, msg_scan sc, const msg3* __restrict__ total,
                                                  const uint64_t* __restrict__ counts,
                                                  const dmsg_state* __restrict__ state_in,
                                                  const dmsg* __restrict__ msgs, uint64_t* __restrict__ seg_first,
                                                  uint64_t* __restrict__ seg_count, dmsg_state* __restrict__ state_out) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= in.nseg) return;
    const uint64_t nrec = in.nrec();
    const uint64_t b = in.bases[s];
    uint64_t cnt = counts[s];
    if (b >= nrec) cnt = 0;
    else if (cnt > nrec - b) cnt = nrec - b;
    dmsg_state st = dmsg_state{0, 0, 0};
    if (state_in) st = state_in[s];
    if (cnt == 0) {   // no records: no pieces, the state unchanged
        seg_first[s] = b < nrec ? sc(b).close : total->close;
        seg_count[s] = 0;
        state_out[s] = st;
        return;
    }
    const uint64_t last = b + cnt - 1;
    const msg3 e = sc(last), own = in(last);
    const uint64_t first = sc(b).close;
    seg_first[s] = first;
    seg_count[s] = e.close + 1 - first;   // the last record closes a piece
    const uint64_t latch = e.latch > own.latch ? e.latch : own.latch;
    dmsg_state o;
    o.opcode = latch > b ? in.info[latch - 1] & F_OPMASK : st.opcode;
    if (msg_load::fin_end(in.info[last])) {
        o.open = 0;
        o.pending = 0;
    } else {   // the trailing open piece; its total includes what was pending when it is the only one
        o.open = 1;
        o.pending = msgs[e.close].total;
    }
    state_out[s] = o;
}

// k_msg_segs over rows; carry_off[s]: where the segment's trailing open piece
// begins in the output (0 when nothing is pending).
__global__ __launch_bounds__(256) void k_join_segs(row_load in, msg_scan sc, const uint64_t* __restrict__ counts,
                                                   const dmsg_state* __restrict__ state_in,
                                                   const dmsg* __restrict__ msgs, uint64_t* __restrict__ seg_first,
                                                   uint64_t* __restrict__ seg_count, dmsg_state* __restrict__ state_out,
                                                   uint64_t* __restrict__ carry_off) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= in.nseg) return;
    const uint64_t nrec = in.records();
    const uint64_t rb = in.bases[s];
    uint64_t cnt = counts[s];
    if (rb >= nrec) cnt = 0;
    else if (cnt > nrec - rb) cnt = nrec - rb;
    dmsg_state st = dmsg_state{0, 0, 0};
    if (state_in) st = state_in[s];
    const uint64_t b = in.base(s);
    const uint64_t first = sc(b).close;
    seg_first[s] = first;
    if (cnt == 0) {   // no records: the state unchanged; carried bytes are one open piece
        seg_count[s] = st.pending ? 1 : 0;
        state_out[s] = st;
        carry_off[s] = st.pending ? msgs[first].off : 0;
        return;
    }
    const uint64_t last = b + cnt;
    const msg3 e = sc(last), own = in(last);
    seg_count[s] = e.close + 1 - first;   // the last row closes a piece
    const uint64_t latch = e.latch > own.latch ? e.latch : own.latch;
    dmsg_state o;
    o.opcode = latch > b ? in.inf(latch - 1) & F_OPMASK : st.opcode;
    uint64_t off = 0;
    if (row_load::fin_end(in.inf(last))) {
        o.open = 0;
        o.pending = 0;
    } else {   // the trailing open piece: its len holds the carried bytes when it is the only one
        o.open = 1;
        o.pending = msgs[e.close].total;
        if (o.pending) off = msgs[e.close].off;
    }
    state_out[s] = o;
    carry_off[s] = off;
}

// k_join_segs over the two virtual connections of each connection: first /
// count cover both classes (data pieces, then control pieces); state_out is
// hvws_rfc_state, each class's offset being where its trailing open piece
// begins in the output (0 when nothing is pending).
__global__ __launch_bounds__(256) void k_rfc_segs(rfc_load in, msg_scan sc, const uint64_t* __restrict__ vcnt,
                                                  const dmsg_state* __restrict__ vstate_in,
                                                  const dmsg* __restrict__ msgs, uint64_t* __restrict__ seg_first,
                                                  uint64_t* __restrict__ seg_count, drfc_state* __restrict__ state_out) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (2u * s >= in.nseg) return;
    drfc_state out;
    uint64_t pieces = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < 2; ++j) {
        const uint32_t v = 2u * s + j;
        const uint64_t b = in.base(v), cnt = vcnt[v];
        dmsg_state st = dmsg_state{0, 0, 0};
        if (vstate_in) st = vstate_in[v];
        const uint64_t first = sc(b).close;
        if (j == 0) seg_first[s] = first;
        dmsg_state o = st;
        uint64_t off = 0;
        if (cnt == 0) {   // no records: the state unchanged; carried bytes are one open piece
            pieces += st.pending ? 1 : 0;
            if (st.pending) off = msgs[first].off;
        } else {
            const uint64_t last = b + cnt;
            const msg3 e = sc(last), own = in(last);
            pieces += e.close + 1 - first;   // the class's last row closes a piece
            const uint64_t latch = e.latch > own.latch ? e.latch : own.latch;
            o.opcode = latch > b ? in.inf(latch - 1) & F_OPMASK : st.opcode;
            if (rfc_load::fin_end(in.inf(last))) {
                o.open = 0;
                o.pending = 0;
            } else {
                o.open = 1;
                o.pending = msgs[e.close].total;
                if (o.pending) off = msgs[e.close].off;
            }
        }
        if (j == 0) {
            out.data = o;
            out.data_off = off;
        } else {
            out.ctl = o;
            out.ctl_off = off;
        }
    }
    seg_count[s] = pieces;
    state_out[s] = out;
}

// ------------------------------------------------------------ k_msg_gather

// Two geometries (threads x chunks of 16 B per thread), by the batch's mean
// bytes per record ($HVWS_EXPERIMENT msg = 0 / 1 fixes one):
//   0  256 x 4, 16 KiB tiles, up to 512 records staged; boundary tiles build
//      their chunks one at a time (56 VGPRs, 8 waves per SIMD).  For frames
//      below 4 KiB, where every tile holds record boundaries.
//   1  one wave per tile of 64 x 4 chunks (4 KiB): no barrier across waves,
//      and with 64 KiB frames only 1 tile in 16 holds a record boundary (the
//      transmit side's k_build<64x4> geometry); boundary tiles
//      issue the loads of all their one-record chunks first (126 VGPRs, 4
//      waves per SIMD, no scratch; asked for 5, 6 or 8 waves per SIMD the
//      compiler spilled 196-324 bytes per lane, so the kernel carries no
//      occupancy attribute).
// Measured on one box (scripts/bench_messages.py, profiles/messages_raw): c3
// 23.7 ms with geometry 0, 20.6-21.3 ms with 1; c2 0.48-0.50 ms with 0,
// 0.59-0.61 ms with 1.
template <int G>
struct msg_geom;
template <>
struct msg_geom<0> {
    static constexpr int T = 256, U = 4;
    static constexpr uint32_t MAXF = 512;   // records staged in LDS per tile
    static constexpr bool AHEAD = false;
};
template <>
struct msg_geom<1> {
    static constexpr int T = 64, U = 4;
    static constexpr uint32_t MAXF = 128;
    static constexpr bool AHEAD = true;
};
static_assert(MSG_TILE == 256 * 4 * 16 && MSG_TILE % (64 * 4 * 16) == 0, "MSG_TILE: a multiple of every geometry's tile");

// first record of a tile's k = 0 .. nf - 1 ending after output offset c
template <typename END>
__device__ __forceinline__ uint32_t msg_find(uint64_t c, uint32_t nf, END endf) {
    uint32_t i = 0, hi = nf;
    while (i < hi) {
        const uint32_t mid = (i + hi) >> 1;
        if (endf(mid) > c) hi = mid;
        else i = mid + 1;
    }
    return i;
}

// Output chunk [c, c + 16) from record i on (output offset offf(k), output
// end endf(k), source offset srcf(k), key word for aligned source words
// keyf(k)), piece by piece; bytes at or beyond `total` are not written.
// J (the joined form): a source offset with ROW_PREV lies in prev, and no read
// leaves [prev, prev + prev_len).
template <bool J>
__device__ __forceinline__ const uint8_t* msg_source(const uint8_t* rx, uint64_t rx_len, const uint8_t* prev,
                                                     uint64_t prev_len, uint64_t& q, uint64_t& bound) {
    if constexpr (J) {
        if (q & ROW_PREV) {
            q &= ~ROW_PREV;
            bound = prev_len;
            return prev;
        }
    }
    bound = rx_len;
    return rx;
}

template <bool J, typename OFF, typename END, typename SRC, typename KEY>
__device__ __forceinline__ void msg_walk(const uint8_t* __restrict__ rx, uint64_t rx_len,
                                         const uint8_t* __restrict__ prev, uint64_t prev_len,
                                         uint8_t* __restrict__ out, uint64_t total, uint64_t c, uint32_t i, uint32_t nf,
                                         OFF offf, END endf, SRC srcf, KEY keyf) {
    uint64_t lo = 0, hh = 0;
#pragma unroll 1
    for (; i < nf; ++i) {
        const uint64_t o = offf(i), e = endf(i);
        if (o >= c + 16) break;
        if (e <= o) continue;   // a record of 0 bytes
        const uint64_t pb = o > c ? o : c, pe = e < c + 16 ? e : c + 16;
        uint64_t q = srcf(i), bound;
        const uint8_t* from = msg_source<J>(rx, rx_len, prev, prev_len, q, bound);
        q += pb - o;
        uint64_t vlo, vhi;
        ld16_any(from, bound, q, vlo, vhi);
        const uint32_t kw = rotr32(keyf(i), 8u * (uint32_t)(q & 3u));
        const uint64_t kk = (uint64_t)kw | ((uint64_t)kw << 32);
        put_bytes(lo, hh, vlo ^ kk, vhi ^ kk, (uint32_t)(pb - c), (uint32_t)(pe - c));
        if (e >= c + 16) break;   // the output is dense: the next record starts at e
    }
    if (c + 16 <= total) {
        __builtin_nontemporal_store(u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hh, (uint32_t)(hh >> 32)},
                                    reinterpret_cast<u32x4*>(out + c));
    } else {
        for (uint32_t b = 0; b < 16 && c + b < total; ++b)
            out[c + b] = (uint8_t)((b < 8 ? lo >> (8u * b) : hh >> (8u * (b - 8u))) & 0xFFu);
    }
}

// The chunks of one tile.  Chunks inside one record stream (the loads of all
// U chunks are issued before the first is used); chunks holding a record
// boundary, and the batch's last partial chunk, walk their pieces afterwards.
template <int T, int U, bool J, typename OFF, typename END, typename SRC, typename KEY>
__device__ __forceinline__ void msg_tile(const uint8_t* __restrict__ rx, uint64_t rx_len,
                                         const uint8_t* __restrict__ prev, uint64_t prev_len,
                                         uint8_t* __restrict__ out, uint64_t total, uint64_t base, uint32_t nf,
                                         OFF offf, END endf, SRC srcf, KEY keyf) {
    const uint32_t tid = threadIdx.x;
    u32x4 w[U], x[U];
    uint32_t kw[U], sft[U], first[U];
    uint32_t fastmask = 0;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const uint64_t c = base + ((uint64_t)i * T + tid) * 16u;
        w[i] = x[i] = u32x4{0, 0, 0, 0};
        kw[i] = sft[i] = 0;
        first[i] = nf;
        if (c >= total) continue;
        const uint32_t j = msg_find(c, nf, endf);
        first[i] = j;
        if (j >= nf) continue;
        const uint64_t o = offf(j);
        uint64_t q = srcf(j), bound;
        const uint8_t* from = msg_source<J>(rx, rx_len, prev, prev_len, q, bound);
        q += c - o;
        if (o <= c && c + 16 <= endf(j) && c + 16 <= total && (q & ~15ull) + 32 <= bound) {
            fastmask |= 1u << i;
            sft[i] = (uint32_t)(q & 15u);
            const u32x4* p = reinterpret_cast<const u32x4*>(from + (q & ~15ull));
            w[i] = p[0];
            if (sft[i]) x[i] = p[1];
            kw[i] = rotr32(keyf(j), 8u * (uint32_t)(q & 3u));
        }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
        if (!((fastmask >> i) & 1u)) continue;
        const uint64_t c = base + ((uint64_t)i * T + tid) * 16u;
        const u32x4 v = (sft[i] ? funnel16(w[i], x[i], sft[i]) : w[i]) ^ u32x4{kw[i], kw[i], kw[i], kw[i]};
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(out + c));
    }
#pragma unroll 1
    for (int i = 0; i < U; ++i) {
        if (((fastmask >> i) & 1u) || first[i] >= nf) continue;
        const uint64_t c = base + ((uint64_t)i * T + tid) * 16u;
        msg_walk<J>(rx, rx_len, prev, prev_len, out, total, c, first[i], nf, offf, endf, srcf, keyf);
    }
}

// J: the tables are the row table's (pay_off = the rows' source words, meta[0]
// = rows); a carried row streams, stages and walks as a record does, from prev.
// The joined instantiations take 58 and 126 VGPRs, no scratch.
template <int G, bool J>
__global__ __launch_bounds__(msg_geom<G>::T) void k_msg_gather(const uint8_t* __restrict__ rx, uint64_t rx_len,
                                                     const uint8_t* __restrict__ prev, uint64_t prev_len,
                                                     const uint64_t* __restrict__ pay_off,
                                                     const uint64_t* __restrict__ pay_len,
                                                     const uint32_t* __restrict__ keyrot,
                                                     const uint64_t* __restrict__ out_off,
                                                     const uint32_t* __restrict__ tile_first,
                                                     const uint64_t* __restrict__ meta, uint32_t masked,
                                                     uint8_t* __restrict__ out, uint64_t out_cap, uint64_t tile0) {
    constexpr int T = msg_geom<G>::T, U = msg_geom<G>::U;
    constexpr uint32_t MAXF = msg_geom<G>::MAXF;
    constexpr uint64_t TILE = (uint64_t)T * U * 16u;
    __shared__ uint64_t s_off[MAXF];
    __shared__ uint64_t s_end[MAXF];
    __shared__ uint64_t s_src[MAXF];
    __shared__ uint32_t s_key[MAXF];

    const uint64_t t = tile0 + blockIdx.x;
    const uint64_t base = t * TILE;
    const uint32_t tid = threadIdx.x;
    const uint64_t nrec = meta[0];
    const uint64_t total = meta[1] < out_cap ? meta[1] : out_cap;
    if (base >= total) return;
    const uint32_t k0 = tile_first[t];
    const uint32_t k1r = tile_first[t + 1];
    const uint32_t k1 = (uint64_t)k1r + 1 < nrec ? k1r + 1 : (uint32_t)nrec;   // records touching the tile: [k0, k1)
    if (k0 >= k1) return;
    const uint32_t nf = k1 - k0;

    // A tile inside one record streams.
    {
        const uint64_t o = out_off[k0], n = pay_len[k0];
        if (o <= base && base + TILE <= o + n && base + TILE <= total) {
            uint64_t src = pay_off[k0], bound;
            const uint8_t* from = msg_source<J>(rx, rx_len, prev, prev_len, src, bound);
            src += base - o;
            const uint64_t src_a = src & ~15ull;
            const uint32_t sft = (uint32_t)(src & 15u);
            if (src_a + TILE + (sft ? 16u : 0u) <= bound) {
                const uint32_t kw = masked ? rotr32(keyrot[k0], 8u * (uint32_t)(src & 3u)) : 0u;
                const u32x4 kv = u32x4{kw, kw, kw, kw};
                const uint8_t* sp = from + src_a;
                u32x4 v[U];
                if (sft == 0) {
#pragma unroll
                    for (int i = 0; i < U; ++i)
                        v[i] = __builtin_nontemporal_load(
                            reinterpret_cast<const u32x4*>(sp + ((uint64_t)i * T + tid) * 16u));
                } else {
                    u32x4 w[U], x[U];
#pragma unroll
                    for (int i = 0; i < U; ++i) {
                        const u32x4* q = reinterpret_cast<const u32x4*>(sp + ((uint64_t)i * T + tid) * 16u);
                        w[i] = q[0];
                        x[i] = q[1];
                    }
#pragma unroll
                    for (int i = 0; i < U; ++i) v[i] = funnel16(w[i], x[i], sft);
                }
#pragma unroll
                for (int i = 0; i < U; ++i)
                    __builtin_nontemporal_store(v[i] ^ kv,
                                                reinterpret_cast<u32x4*>(out + base + ((uint64_t)i * T + tid) * 16u));
                return;
            }
        }
    }

    auto chunk = [&](uint64_t c, auto offf, auto endf, auto srcf, auto keyf) {
        const uint32_t j = msg_find(c, nf, endf);
        if (j < nf) msg_walk<J>(rx, rx_len, prev, prev_len, out, total, c, j, nf, offf, endf, srcf, keyf);
    };
    if (nf <= MAXF) {
        for (uint32_t i = tid; i < nf; i += T) {
            const uint64_t o = out_off[k0 + i];
            s_off[i] = o;
            s_end[i] = o + pay_len[k0 + i];
            s_src[i] = pay_off[k0 + i];
            s_key[i] = masked ? keyrot[k0 + i] : 0u;
        }
        __syncthreads();
        auto offf = [&](uint32_t k) { return s_off[k]; };
        auto endf = [&](uint32_t k) { return s_end[k]; };
        auto srcf = [&](uint32_t k) { return s_src[k]; };
        auto keyf = [&](uint32_t k) { return s_key[k]; };
        if constexpr (msg_geom<G>::AHEAD) {
            msg_tile<T, U, J>(rx, rx_len, prev, prev_len, out, total, base, nf, offf, endf, srcf, keyf);
        } else {
#pragma unroll 1
            for (int i = 0; i < U; ++i) {
                const uint64_t c = base + ((uint64_t)i * T + tid) * 16u;
                if (c >= total) break;
                chunk(c, offf, endf, srcf, keyf);
            }
        }
    } else {   // more records than the LDS area holds (frames of a few bytes): from the tables
#pragma unroll 1
        for (int i = 0; i < U; ++i) {
            const uint64_t c = base + ((uint64_t)i * T + tid) * 16u;
            if (c >= total) break;
            chunk(
                c, [&](uint32_t k) { return out_off[k0 + k]; },
                [&](uint32_t k) { return out_off[k0 + k] + pay_len[k0 + k]; },
                [&](uint32_t k) { return pay_off[k0 + k]; },
                [&](uint32_t k) { return masked ? keyrot[k0 + k] : 0u; });
        }
    }
}

int msg_pick(uint64_t rx_len, uint64_t cap) {
    const char* e = experiment("msg");   // read per call (tests switch it)
    const int forced = e ? atoi(e) : -1;
    if (forced == 0 || forced == 1) return forced;
    return cap && rx_len / cap >= 4096 ? 1 : 0;
}

}  // namespace

uint64_t msg_scratch_bytes(uint64_t cap) { return (cap + 16 + scan_tmp_words(cap)) * sizeof(msg3); }

hipError_t launch_msg_table(const uint64_t* pay_len, const uint32_t* info, const uint64_t* nfr_dev, uint64_t cap,
                            const uint64_t* counts, const uint64_t* bases, uint32_t nseg, const dmsg_state* state_in,
                            void* scratch, uint64_t* out_off, dmsg* msgs, uint64_t* seg_first, uint64_t* seg_count,
                            dmsg_state* state_out, uint64_t* meta, hipStream_t st) {
    msg3* ex = reinterpret_cast<msg3*>(scratch);
    msg3* total = ex + cap;            // one value; 16 are set aside
    msg3* tmp = ex + cap + 16;
    const msg_load in{pay_len, info, nfr_dev, cap, bases, nseg};
    hipError_t e = launch_scan_of(in, ex, cap, tmp, total, st, false);
    if (e != hipSuccess) return e;
    const uint64_t nb = (cap + SCAN_B - 1) / SCAN_B;
    const msg_scan sc{ex, nb > 1 ? tmp + nb : (const msg3*)nullptr};
    const uint32_t rb = (uint32_t)((cap + 255) / 256);
    hipLaunchKernelGGL(k_msg_records<msg_load>, dim3(rb ? rb : 1), dim3(256), 0, st, in, sc, total, out_off, msgs,
                       (uint64_t*)nullptr, meta);
    if (rb)
        hipLaunchKernelGGL(k_msg_pieces<msg_load>, dim3(rb), dim3(256), 0, st, in, sc, total, state_in,
                           (const uint64_t*)nullptr, msgs);
    if (nseg)
        hipLaunchKernelGGL(k_msg_segs, dim3((nseg + 255) / 256), dim3(256), 0, st, in, sc, total, counts, state_in, msgs,
                           seg_first, seg_count, state_out);
    return hipGetLastError();
}

hipError_t launch_msg_table_joined(const dframes& fr, int masked, const uint64_t* nfr_dev, uint64_t cap,
                                   const uint64_t* counts, const uint64_t* bases, uint32_t nseg,
                                   const dmsg_state* state_in, const uint64_t* prev_off, void* scratch,
                                   const msg_rows& rows, uint64_t* out_off, dmsg* msgs, uint64_t* seg_first,
                                   uint64_t* seg_count, dmsg_state* state_out, uint64_t* carry_off, uint64_t* meta,
                                   hipStream_t st) {
    if (nseg == 0) return hipErrorInvalidValue;   // row 0 is segment 0's
    const uint64_t nrows = cap + nseg;
    msg3* ex = reinterpret_cast<msg3*>(scratch);
    msg3* total = ex + nrows;
    msg3* tmp = ex + nrows + 16;
    const row_load in{rows.len, rows.info, nfr_dev, cap, bases, nseg};
    const uint32_t rb = (uint32_t)((nrows + 255) / 256);
    hipLaunchKernelGGL(k_join_rows, dim3(rb), dim3(256), 0, st, in, fr.pay_off, fr.pay_len, fr.info, fr.keyrot,
                       masked ? 1u : 0u, state_in, prev_off, rows.len, rows.src, rows.key, rows.info);
    hipError_t e = launch_scan_of(in, ex, nrows, tmp, total, st, false);
    if (e != hipSuccess) return e;
    const uint64_t nb = (nrows + SCAN_B - 1) / SCAN_B;
    const msg_scan sc{ex, nb > 1 ? tmp + nb : (const msg3*)nullptr};
    hipLaunchKernelGGL(k_msg_records<row_load>, dim3(rb), dim3(256), 0, st, in, sc, total, out_off, msgs, rows.prow,
                       meta);
    hipLaunchKernelGGL(k_msg_pieces<row_load>, dim3(rb), dim3(256), 0, st, in, sc, total, state_in, rows.prow, msgs);
    hipLaunchKernelGGL(k_join_segs, dim3((nseg + 255) / 256), dim3(256), 0, st, in, sc, counts, state_in, msgs,
                       seg_first, seg_count, state_out, carry_off);
    return hipGetLastError();
}

uint64_t msg_cls_bytes(uint64_t cap) { return (cap + 16 + scan_tmp_words(cap)) * sizeof(cls2); }

hipError_t launch_msg_table_rfc(const dframes& fr, int masked, const uint64_t* nfr_dev, uint64_t cap,
                                const uint64_t* bases, uint32_t nseg, const dmsg_state* vstate_in,
                                const uint64_t* voff, void* scratch, void* cls_scratch, const msg_rows& rows,
                                const rfc_rows& rr, uint64_t* out_off, dmsg* msgs, uint64_t* seg_first,
                                uint64_t* seg_count, drfc_state* state_out, uint64_t* meta, hipStream_t st) {
    if (nseg == 0) return hipErrorInvalidValue;   // row 0 is connection 0's
    const uint64_t nrows = cap + 2ull * nseg;
    cls2* cls = reinterpret_cast<cls2*>(cls_scratch);
    cls2* cls_total = cls + cap;   // one value; 16 are set aside
    cls2* cls_tmp = cls + cap + 16;
    hipError_t e = launch_scan_of(cls_load{fr.info, nfr_dev, cap}, cls, cap, cls_tmp, cls_total, st, false);
    if (e != hipSuccess) return e;
    const uint64_t cb = (cap + SCAN_B - 1) / SCAN_B;
    const cls_scan cs{cls, cb > 1 ? cls_tmp + cb : (const cls2*)nullptr, cls_total, cap};
    msg3* ex = reinterpret_cast<msg3*>(scratch);
    msg3* total = ex + nrows;
    msg3* tmp = ex + nrows + 16;
    const uint32_t rb = (uint32_t)((nrows + 255) / 256);
    hipLaunchKernelGGL(k_rfc_rows, dim3(rb), dim3(256), 0, st, nfr_dev, cap, bases, nseg, cs, fr.pay_off,
                       fr.pay_len, fr.info, fr.keyrot, masked ? 1u : 0u, vstate_in, voff, rows.len, rows.src, rows.key,
                       rows.info, rr.rec, rr.vbase, rr.vcnt);
    const rfc_load in{rows.len, rows.info, nfr_dev, cap, rr.vbase, rr.rec, 2u * nseg};
    e = launch_scan_of(in, ex, nrows, tmp, total, st, false);
    if (e != hipSuccess) return e;
    const uint64_t nb = (nrows + SCAN_B - 1) / SCAN_B;
    const msg_scan sc{ex, nb > 1 ? tmp + nb : (const msg3*)nullptr};
    hipLaunchKernelGGL(k_msg_records<rfc_load>, dim3(rb), dim3(256), 0, st, in, sc, total, out_off, msgs, rows.prow,
                       meta);
    hipLaunchKernelGGL(k_msg_pieces<rfc_load>, dim3(rb), dim3(256), 0, st, in, sc, total, vstate_in, rows.prow, msgs);
    hipLaunchKernelGGL(k_rfc_segs, dim3((nseg + 255) / 256), dim3(256), 0, st, in, sc, rr.vcnt, vstate_in, msgs,
                       seg_first, seg_count, state_out);
    return hipGetLastError();
}

uint64_t msg_gather_tile(int g) { return g == 1 ? 64u * 4u * 16u : 256u * 4u * 16u; }
int msg_variant(uint64_t rx_len, uint64_t cap) { return msg_pick(rx_len, cap); }

hipError_t launch_msg_gather(int g, const uint8_t* rx, uint64_t rx_len, const uint64_t* pay_off,
                             const uint64_t* pay_len, const uint32_t* keyrot, const uint64_t* out_off,
                             const uint32_t* tile_first, uint64_t ntiles, const uint64_t* meta, int masked,
                             uint8_t* out, uint64_t out_cap, hipStream_t st) {
    // a grid beyond 2^32-1 work-items is silently truncated: split the launch
    const uint64_t per_launch = 0xFFFFFFFFull / 256;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += per_launch) {
        const uint64_t nt = ntiles - t0 < per_launch ? ntiles - t0 : per_launch;
        if (g == 1)
            hipLaunchKernelGGL((k_msg_gather<1, false>), dim3((uint32_t)nt), dim3(msg_geom<1>::T), 0, st, rx, rx_len,
                               (const uint8_t*)nullptr, (uint64_t)0, pay_off, pay_len, keyrot, out_off, tile_first, meta,
                               masked ? 1u : 0u, out, out_cap, t0);
        else
            hipLaunchKernelGGL((k_msg_gather<0, false>), dim3((uint32_t)nt), dim3(msg_geom<0>::T), 0, st, rx, rx_len,
                               (const uint8_t*)nullptr, (uint64_t)0, pay_off, pay_len, keyrot, out_off, tile_first, meta,
                               masked ? 1u : 0u, out, out_cap, t0);
    }
    return hipGetLastError();
}

hipError_t launch_msg_gather_joined(int g, const uint8_t* rx, uint64_t rx_len, const uint8_t* prev, uint64_t prev_len,
                                    const msg_rows& rows, const uint64_t* out_off, const uint32_t* tile_first,
                                    uint64_t ntiles, const uint64_t* meta, int masked, uint8_t* out, uint64_t out_cap,
                                    hipStream_t st) {
    const uint64_t per_launch = 0xFFFFFFFFull / 256;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += per_launch) {
        const uint64_t nt = ntiles - t0 < per_launch ? ntiles - t0 : per_launch;
        if (g == 1)
            hipLaunchKernelGGL((k_msg_gather<1, true>), dim3((uint32_t)nt), dim3(msg_geom<1>::T), 0, st, rx, rx_len, prev,
                               prev_len, rows.src, rows.len, rows.key, out_off, tile_first, meta, masked ? 1u : 0u, out,
                               out_cap, t0);
        else
            hipLaunchKernelGGL((k_msg_gather<0, true>), dim3((uint32_t)nt), dim3(msg_geom<0>::T), 0, st, rx, rx_len, prev,
                               prev_len, rows.src, rows.len, rows.key, out_off, tile_first, meta, masked ? 1u : 0u, out,
                               out_cap, t0);
    }
    return hipGetLastError();
}

}  // namespace hvws
