// k_interaction.hpp — the INTERACTION (logup) columns of the recursion circuit's two components for a batch of proofs
// (rsv_witness_interaction_dev, interaction_api.inc): tree 2 of the next proof, from the trace columns k_trace.hpp wrote,
// the program's preprocessed columns and the next proof's lookup elements (z, alpha).
//
// The AIR (components/recursive/composition/src/{data_structures,plonk,poseidon}.rs)
// adds relation entries multiplicity / (sum_i alpha^i values[i] - z) and batches them: Plonk {a, b}, {c, poseidon};
// Poseidon {3 entries}, {2 entries}.  Per component, f0 / f1 = the two batches' fraction sums at a row, and
//   column 0 (M31 columns 0..3) = f0,
//   column 1 (M31 columns 4..7) = S[k] = sum_{j <= k} (f0[j] + f1[j] - shift), shift = total / 2^n, total = the claimed
//     sum, k the COSET index (stwo's finalize_last / inclusive_prefix_sum), so S[last] = 0.
// Rows are stored like the trace: position i = 2 m + b holds circle-domain index bitrev_n(i), whose coset index is
// 2 r (b = 0) or N - 1 - 2 r (b = 1), r = bitrev_{n-1}(m).
//
// The prefix sum without uncoalesced traffic.  Split m = X * 2^B + L (X: s = n - 1 - B high bits).  Coset chunk c
// (2^(s+1) consecutive k, c < 2^B) holds, at its step v < 2^s, the even row of m = (bitrev_s(v), bitrev_B(c)) and then the
// odd row of m = (~bitrev_s(v), ~bitrev_B(c)).  So chunks are COLUMNS of the [X][L] matrix, and a lane that owns column L
// (forward through chunk c(L)) and column ~L (BACKWARD through chunk c(~L), from its known end) touches, at every step,
// the row pairs (X, L) and (~X, ~L) whole: every read and write of a wave is a contiguous 512-byte run.
//   k_int_prep     one lane per proof: (z, alpha, alpha^2) reduced once, the zero-denominator flag cleared.
//   k_int_frac     one lane per (row, proof): the fractions, column 0, and f0 + f1 parked in column 1.
//   k_int_chunks   one lane per (proof, L < 2^(B-1)): the sums of chunks c(L) and c(~L).
//   k_int_offsets  one workgroup of 1 024 per (proof, component), 4 chunks per thread: the chunk sums scanned (registers,
//                  then wave shuffles, then the 16 wave totals), the claimed sum, the shifted start / end of every chunk,
//                  d_sums and d_ok.
//   k_int_scan     one lane per (proof, L): column 1 in place (forward and backward), or zeros.
// Every phase is ONE launch for both components (blockIdx.y = component): five launches per call.  B adapts to the
// batch (interaction_api.inc): 2^(B-1) scan lanes per (proof, component), B <= 12 — 2 x 2 048 scan lanes for one
// proof, about 2^17 from 32 proofs on; the fraction kernel always has one lane per row.
//
// Inversions: one q_inv per row, shared by the row's 4 (Plonk) or 5 (Poseidon) denominators (Montgomery's trick inside
// the row: 1 / (q0 q1), then f0 = p0 q1 / (q0 q1), f1 = p1 q0 / (q0 q1)).  A longer chain across rows would not pay: the
// QM31 inverse is one M31 inverse (37 products) plus a few CM31 products, about 3.3 QM31 products, and every further row
// in a chain costs 3.  A row with a zero denominator has d = q0 q1 = 0: it marks its proof (d_ok = 0, zero output) and
// nothing else, since no inverse is shared across rows.
#pragma once
#include "field.hpp"
#include "trace_host.hpp"

namespace rsv {

constexpr uint32_t INT_COLS = 8;       // M31 columns per component
constexpr uint32_t INT_MAX_B = 12;     // at most 4 096 chunks per (proof, component): 4 per thread of k_int_offsets
constexpr uint32_t INT_OFF_THREADS = 1024;

// Per component.
struct IntComp {
    const uint32_t* pre;      // [10 | 40][2^log]: the component's preprocessed columns (rsv_trace_preprocessed)
    const uint32_t* trace;    // [n][n_trace][2^log]
    uint32_t n_trace, log, B;
    uint32_t* out;            // [n][8][2^log]
    uint4* start;             // [n][2^B]: by L, the shifted exclusive prefix at the start of chunk c(L)
    uint4* end;               // [n][2^B]: by L, the shifted inclusive prefix at the end of chunk c(L)
    uint4* shift;             // [n]
    uint32_t* sums;           // [n][2][4] + component * 4
};

struct IntArgs {
    const uint8_t* accept;    // [n]
    const uint32_t* lookup;   // [n][8]: z, alpha as given
    uint4* lk;                // [n][3]: z, alpha, alpha^2, canonical (k_int_prep)
    uint32_t n;
    uint32_t* bad;            // [n]: a zero denominator (cleared by k_int_prep)
    uint8_t* ok;              // [n] or NULL
    IntComp c[2];             // Plonk, Poseidon
};

__device__ __forceinline__ uint32_t brev(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32u - bits) : 0u; }
__device__ __forceinline__ QM31 q_of4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return q_mk(a, b, c, d); }
__device__ __forceinline__ uint4 q_u4(QM31 x) { return make_uint4(x.a.a, x.a.b, x.b.a, x.b.b); }
__device__ __forceinline__ QM31 u4_q(uint4 v) { return q_mk(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ bool q_is_zero(QM31 x) { return ((x.a.a | x.a.b) | (x.b.a | x.b.b)) == 0; }
// v0 + alpha v1 - z with v0, v1 in M31
__device__ __forceinline__ QM31 den_mm(uint32_t v0, uint32_t v1, QM31 alpha, QM31 z) {
    return q_sub(q_add(q_from_m(v0), q_mul_m(alpha, v1)), z);
}
// v0 + alpha v1 + alpha^2 v2 - z with v0 in M31
__device__ __forceinline__ QM31 den_mqq(uint32_t v0, QM31 v1, QM31 v2, QM31 alpha, QM31 alpha2, QM31 z) {
    return q_sub(q_add(q_from_m(v0), q_add(q_mul(alpha, v1), q_mul(alpha2, v2))), z);
}

// Writes f0 to columns 0..3 and f0 + f1 to columns 4..7 of row i; marks the proof on a zero denominator.
__device__ __forceinline__ void int_finish(QM31 p0, QM31 q0, QM31 p1, QM31 q1, uint32_t* out, size_t N, size_t i, uint32_t* bad) {
    const QM31 d = q_mul(q0, q1);
    if (q_is_zero(d)) *bad = 1u;
    const QM31 inv = q_inv(d);
    const QM31 f0 = q_mul(p0, q_mul(q1, inv)), f1 = q_mul(p1, q_mul(q0, inv));
    const QM31 g = q_add(f0, f1);
    out[0 * N + i] = f0.a.a; out[1 * N + i] = f0.a.b; out[2 * N + i] = f0.b.a; out[3 * N + i] = f0.b.b;
    out[4 * N + i] = g.a.a;  out[5 * N + i] = g.a.b;  out[6 * N + i] = g.b.a;  out[7 * N + i] = g.b.b;
}

// One lane per proof, before everything else: the per-proof constants, so that no row lane reduces or squares them.
__global__ __launch_bounds__(256) void k_int_prep(IntArgs a) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t* w = a.lookup + 8 * (size_t)p;
    const QM31 z = q_mk(w[0] % P, w[1] % P, w[2] % P, w[3] % P), alpha = q_mk(w[4] % P, w[5] % P, w[6] % P, w[7] % P);
    a.lk[3 * (size_t)p + 0] = q_u4(z);
    a.lk[3 * (size_t)p + 1] = q_u4(alpha);
    a.lk[3 * (size_t)p + 2] = q_u4(q_mul(alpha, alpha));
    a.bad[p] = 0;
}

// ---------------------------------------------------------------- fractions
// Plonk preprocessed: a_wire, b_wire, c_wire, mult_a, mult_b, mult_c, poseidon_wire, mult_poseidon.
__device__ __forceinline__ void int_plonk_row(const IntComp& c, const uint32_t* t, const uint32_t* w, size_t N, QM31 z, QM31 alpha,
                                              QM31 alpha2, QM31& p0, QM31& q0, QM31& p1, QM31& q1) {
    using namespace trace;
    const QM31 av = q_of4(t[0], t[N], t[2 * N], t[3 * N]), bv = q_of4(t[4 * N], t[5 * N], t[6 * N], t[7 * N]);
    const QM31 cv = q_of4(t[8 * N], t[9 * N], t[10 * N], t[11 * N]);
    const QM31 qa = q_sub(q_add(av, q_mul_m(alpha, w[PLONK_A_WIRE * N])), z);
    const QM31 qb = q_sub(q_add(bv, q_mul_m(alpha, w[PLONK_B_WIRE * N])), z);
    const QM31 qc = q_sub(q_add(cv, q_mul_m(alpha, w[PLONK_C_WIRE * N])), z);
    const QM31 qp = den_mqq(w[PLONK_POSEIDON_WIRE * N], av, bv, alpha, alpha2, z);
    p0 = q_add(q_mul_m(qb, w[PLONK_MULT_A * N]), q_mul_m(qa, w[PLONK_MULT_B * N]));
    p1 = q_add(q_mul_m(qp, w[PLONK_MULT_C * N]), q_mul_m(qc, m_neg(w[PLONK_MULT_POSEIDON * N])));
    q0 = q_mul(qa, qb);
    q1 = q_mul(qc, qp);
}

// Poseidon preprocessed: is_first, is_last, round_id, rc0[0] (the swap address), external_idx_1, external_idx_2,
// is_external_idx_1_nonzero, is_external_idx_2_nonzero.  Trace: in[16], intermediate[16], out[16].
__device__ __forceinline__ void int_poseidon_row(const IntComp& c, const uint32_t* t, const uint32_t* w, size_t N, QM31 z, QM31 alpha,
                                                 QM31 alpha2, QM31& p0, QM31& q0, QM31& p1, QM31& q1) {
    using namespace trace;
    const uint32_t first = w[POSEIDON_IS_FIRST * N], last = w[POSEIDON_IS_LAST * N], rid2 = m_dbl(w[POSEIDON_ROUND_ID * N]);
    const uint32_t addr = w[POSEIDON_SWAP_ADDR * N], ext1 = w[POSEIDON_EXT_WIRE_1 * N], ext2 = w[POSEIDON_EXT_WIRE_2 * N];
    const uint32_t nz1 = w[POSEIDON_EXT_NZ_1 * N], nz2 = w[POSEIDON_EXT_NZ_2 * N];
    const uint32_t nf = m_sub(1, first), nl = m_sub(1, last);
    auto st = [&](int k) { return q_of4(t[(size_t)k * N], t[(size_t)(k + 1) * N], t[(size_t)(k + 2) * N], t[(size_t)(k + 3) * N]); };
    // in_left, in_right: ids 2 round_id (+1) unless the first round (the external wire)
    const QM31 e1 = den_mqq(m_add(m_mul(first, ext1), m_mul(nf, rid2)), st(0), st(4), alpha, alpha2, z);
    const QM31 e2 = den_mqq(m_add(m_mul(first, ext2), m_mul(nf, m_add(rid2, 1))), st(8), st(12), alpha, alpha2, z);
    const QM31 e3 = den_mqq(m_add(m_mul(last, ext1), m_mul(nl, m_add(rid2, 2))), st(32), st(36), alpha, alpha2, z);
    const QM31 e4 = den_mqq(m_add(m_mul(last, ext2), m_mul(nl, m_add(rid2, 3))), st(40), st(44), alpha, alpha2, z);
    const QM31 e5 = den_mm(t[(size_t)16 * N], addr, alpha, z);
    const uint32_t m1 = m_sub(m_mul(nz1, first), nf), m2 = m_sub(m_mul(nz2, first), nf);
    const uint32_t m3 = m_add(m_mul(nz1, last), nl), m4 = m_add(m_mul(nz2, last), nl), m5 = m_mul(first, nl);
    const QM31 e12 = q_mul(e1, e2);
    p0 = q_add(q_mul(q_add(q_mul_m(e2, m1), q_mul_m(e1, m2)), e3), q_mul_m(e12, m3));
    p1 = q_add(q_mul_m(e5, m4), q_mul_m(e4, m5));
    q0 = q_mul(e12, e3);
    q1 = q_mul(e4, e5);
}

// Grid (proof-major blocks of 256 rows, component).  A rejected proof is skipped: k_int_scan zeroes it.  (z, alpha,
// alpha^2) are per-proof constants at a workgroup-uniform address: scalar loads.
__global__ __launch_bounds__(256) void k_int_frac(IntArgs a) {
    const IntComp& c = a.c[blockIdx.y];
    const uint32_t N = 1u << c.log, per = (N + 255) / 256;
    const uint32_t p = blockIdx.x / per, i = (blockIdx.x % per) * 256 + threadIdx.x;
    if (p >= a.n || i >= N || !a.accept[p]) return;
    const QM31 z = u4_q(a.lk[3 * (size_t)p]), alpha = u4_q(a.lk[3 * (size_t)p + 1]), alpha2 = u4_q(a.lk[3 * (size_t)p + 2]);
    const uint32_t* t = c.trace + (size_t)p * c.n_trace * N + i;
    const uint32_t* w = c.pre + i;
    QM31 p0, q0, p1, q1;
    if (blockIdx.y == 0) int_plonk_row(c, t, w, N, z, alpha, alpha2, p0, q0, p1, q1);
    else int_poseidon_row(c, t, w, N, z, alpha, alpha2, p0, q0, p1, q1);
    int_finish(p0, q0, p1, q1, c.out + (size_t)p * INT_COLS * N, N, i, a.bad + p);
}

// ---------------------------------------------------------------- the prefix sum in coset order
// Row pair (X, L) of component column `col`: the QM31 at positions 2 m and 2 m + 1, m = X 2^B + L.
__device__ __forceinline__ void pair_ld(const uint32_t* col, size_t N, size_t m, QM31& e, QM31& o) {
    uint2 w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = *reinterpret_cast<const uint2*>(col + k * N + 2 * m);
    e = q_mk(w[0].x, w[1].x, w[2].x, w[3].x);
    o = q_mk(w[0].y, w[1].y, w[2].y, w[3].y);
}
__device__ __forceinline__ void pair_st(uint32_t* col, size_t N, size_t m, QM31 e, QM31 o) {
    *reinterpret_cast<uint2*>(col + 0 * N + 2 * m) = make_uint2(e.a.a, o.a.a);
    *reinterpret_cast<uint2*>(col + 1 * N + 2 * m) = make_uint2(e.a.b, o.a.b);
    *reinterpret_cast<uint2*>(col + 2 * N + 2 * m) = make_uint2(e.b.a, o.b.a);
    *reinterpret_cast<uint2*>(col + 3 * N + 2 * m) = make_uint2(e.b.b, o.b.b);
}

// Grid (proof-major blocks of 64 lanes, component), 2^(B-1) lanes per proof.  Chunk c(L) = even rows of column L + odd
// rows of ~L.
__global__ __launch_bounds__(64) void k_int_chunks(IntArgs a) {
    const IntComp& c = a.c[blockIdx.y];
    const uint32_t half = 1u << (c.B - 1), per = (half + 63) / 64;
    const uint32_t p = blockIdx.x / per, L = (blockIdx.x % per) * 64 + threadIdx.x;
    if (p >= a.n || L >= half || !a.accept[p]) return;
    const size_t N = (size_t)1 << c.log;
    const uint32_t s = c.log - 1 - c.B, Lc = L ^ ((1u << c.B) - 1);
    const uint32_t* g = c.out + (size_t)p * INT_COLS * N + 4 * N;
    QM31 tl = q_zero(), tc = q_zero();
    for (uint32_t X = 0; X < (1u << s); X++) {
        QM31 e, o, ec, oc;
        pair_ld(g, N, ((size_t)X << c.B) + L, e, o);
        pair_ld(g, N, ((size_t)X << c.B) + Lc, ec, oc);
        tl = q_add(tl, q_add(e, oc));
        tc = q_add(tc, q_add(ec, o));
    }
    c.start[((size_t)p << c.B) + L] = q_u4(tl);
    c.start[((size_t)p << c.B) + Lc] = q_u4(tc);
}

__device__ __forceinline__ QM31 q_shfl_up(QM31 x, uint32_t d) {
    return q_mk(__shfl_up(x.a.a, d), __shfl_up(x.a.b, d), __shfl_up(x.b.a, d), __shfl_up(x.b.b, d));
}

// Grid (proof, component), 1 024 threads.  Thread t owns chunks 4 t .. 4 t + 3 in CHUNK order (c = bitrev_B(L)): four
// independent 16-byte loads of start[bitrev(c)] (the 2^B sums are 64 KB at most, L2 / MALL resident), an inclusive scan
// in registers, the thread totals scanned with wave shuffles, the 16 wave totals through LDS.  Each chunk's shifted
// prefix is written back by L: start = E'[c], end = E'[c + 1] = E'[c] + sum(c) - 2^(log - B) shift (0 for the last
// chunk: S[last] = 0).
__global__ __launch_bounds__(INT_OFF_THREADS) void k_int_offsets(IntArgs a) {
    __shared__ uint4 wave_tot[INT_OFF_THREADS / 64];
    const uint32_t comp = blockIdx.y;
    const IntComp& c = a.c[comp];
    const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, C = 1u << c.B;
    const bool ok = a.accept[p] && !a.bad[p];
    if (comp == 0 && a.ok && tid == 0) a.ok[p] = ok;
    uint4* start = c.start + ((size_t)p << c.B);
    uint4* end = c.end + ((size_t)p << c.B);
    if (!ok) {
        if (tid == 0) {
            c.shift[p] = make_uint4(0, 0, 0, 0);
            for (int k = 0; k < 4; k++) c.sums[8 * (size_t)p + k] = 0;
        }
        return;  // k_int_scan zeroes the columns
    }
    QM31 x[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t cc = 4 * tid + j;
        x[j] = cc < C ? u4_q(start[brev(cc, c.B)]) : q_zero();
    }
    QM31 run = q_add(q_add(x[0], x[1]), q_add(x[2], x[3]));
    // inclusive scan of the thread totals inside the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const QM31 up = q_shfl_up(run, d);
        if (lane >= d) run = q_add(run, up);
    }
    if (lane == 63) wave_tot[wv] = q_u4(run);
    __syncthreads();
    QM31 before = q_zero(), total = q_zero();
#pragma unroll
    for (uint32_t k = 0; k < INT_OFF_THREADS / 64; k++) {
        const QM31 t = u4_q(wave_tot[k]);
        if (k < wv) before = q_add(before, t);
        total = q_add(total, t);
    }
    const QM31 shift = q_mul_m(total, 1u << (31 - c.log));  // 1 / 2^log = 2^(31 - log) mod P
    const QM31 wshift = q_mul_m(shift, 1u << (c.log - c.B)); // one chunk's share: 2^(log - B) < 2^31
    // the exclusive prefix of this thread's first chunk: the wave's lanes before it, the waves before it
    QM31 acc = q_add(before, q_sub(run, q_add(q_add(x[0], x[1]), q_add(x[2], x[3]))));
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t cc = 4 * tid + j;
        if (cc < C) {
            // E'[cc] = E[cc] - cc 2^(log - B) shift; cc 2^(log - B) < 2^log <= 2^30
            const QM31 e = q_sub(acc, q_mul_m(shift, cc << (c.log - c.B)));
            const uint32_t L = brev(cc, c.B);
            start[L] = q_u4(e);
            end[L] = q_u4(q_sub(q_add(e, x[j]), wshift));
        }
        acc = q_add(acc, x[j]);
    }
    if (tid == 0) {
        c.shift[p] = q_u4(shift);
        c.sums[8 * (size_t)p + 0] = total.a.a; c.sums[8 * (size_t)p + 1] = total.a.b;
        c.sums[8 * (size_t)p + 2] = total.b.a; c.sums[8 * (size_t)p + 3] = total.b.b;
    }
}

// Grid as k_int_chunks.  Step u: X = bitrev_s(u).  Forward through chunk c(L): the even row of (X, L), then the odd row of
// (~X, ~L).  Backward through chunk c(~L), whose step is 2^s - 1 - u: its odd row (X, L) holds the running sum before
// that row's term is taken off, then its even row (~X, ~L).  A proof that is not ok gets zeros in all 8 columns.
__global__ __launch_bounds__(64) void k_int_scan(IntArgs a) {
    const IntComp& c = a.c[blockIdx.y];
    const uint32_t half = 1u << (c.B - 1), per = (half + 63) / 64;
    const uint32_t p = blockIdx.x / per, L = (blockIdx.x % per) * 64 + threadIdx.x;
    if (p >= a.n || L >= half) return;
    const size_t N = (size_t)1 << c.log;
    const uint32_t s = c.log - 1 - c.B, Lc = L ^ ((1u << c.B) - 1), Xmask = (1u << s) - 1;
    uint32_t* col0 = c.out + (size_t)p * INT_COLS * N;
    uint32_t* g = col0 + 4 * N;
    if (!a.accept[p] || a.bad[p]) {
        const QM31 zz = q_zero();
        for (uint32_t X = 0; X <= Xmask; X++) {
            const size_t mA = ((size_t)X << c.B) + L, mB = ((size_t)X << c.B) + Lc;
            pair_st(col0, N, mA, zz, zz); pair_st(g, N, mA, zz, zz);
            pair_st(col0, N, mB, zz, zz); pair_st(g, N, mB, zz, zz);
        }
        return;
    }
    const QM31 shift = u4_q(c.shift[p]);
    QM31 fwd = u4_q(c.start[((size_t)p << c.B) + L]), bwd = u4_q(c.end[((size_t)p << c.B) + Lc]);
    for (uint32_t u = 0; u <= Xmask; u++) {
        const uint32_t X = brev(u, s);
        const size_t mA = ((size_t)X << c.B) + L, mB = ((size_t)(X ^ Xmask) << c.B) + Lc;
        QM31 ae, ao, be, bo;
        pair_ld(g, N, mA, ae, ao);
        pair_ld(g, N, mB, be, bo);
        fwd = q_add(fwd, q_sub(ae, shift));
        const QM31 sae = fwd;
        fwd = q_add(fwd, q_sub(bo, shift));
        const QM31 sbo = fwd;
        const QM31 sao = bwd;
        bwd = q_sub(bwd, q_sub(ao, shift));
        const QM31 sbe = bwd;
        bwd = q_sub(bwd, q_sub(be, shift));
        pair_st(g, N, mA, sae, sao);
        pair_st(g, N, mB, sbe, sbo);
    }
}

}  // namespace rsv
