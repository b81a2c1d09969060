// k_composition.hpp — tree 3 of the next proof: the composition polynomial of the recursion circuit's two components
// (composition_api.inc drives the launches; include/rsv.h: rsv_composition_dev, rsv_witness_tree3_dev).
//
// With clb = max(lp + 2, lq + 3), every column of both components is extended to CanonicCoset(clb).circle_domain() by the
// commitment's own interpolation and forward FFT (k_commit.hpp), and one lane per extended row evaluates the accumulator
// of CompositionCheck::compute (components/recursive/composition/src/lib.rs:34-121, as k_oods.hpp evaluates it at the OODS point)
// at that row's domain point p:
//   A(p) = 1/Z_lp(p) * sum_{i<6} plonk_i rc^(85-i)  +  1/Z_lq(p) * sum_{j<80} poseidon_j rc^(79-j),   Z_l(p) = pi^(l-1)(p.x),
// which is acc = acc * rc + constraint / Z over the 86 constraints in the reference's order.  At a domain point every column
// value is an M31 word, so the Poseidon round constraints (and Plonk's first three) are M31 arithmetic and their products
// with the wave-uniform powers of rc are four multiply-adds each into unreduced u64 sums (co_add, as k_sp_dot's); only
// the logup constraints, with z, alpha and the combined a / b / c of the Plonk gate, are QM31.  1/Z_l takes 2^(clb - l)
// distinct values on the domain (k_co_zinv's table) and is applied once per component.
//
// Previous row.  Position r (bit-reversed storage) carries the point of natural index i = bitrev_clb(r): i < 2^(clb-1) is
// half_odds(clb-1).at(i) = (2^(30-clb) + i 2^(32-clb)) GEN, i >= 2^(clb-1) the conjugate of i - 2^(clb-1).  The step of
// CanonicCoset(l) is 2^(31-l) GEN = 2^(clb-l-1) index steps, so the previous row is i - 2^(clb-l-1) in the first half and
// i + 2^(clb-l-1) in the conjugate half, modulo 2^(clb-1).  Bit clb-l-1 of i is bit l of r and the carries run towards
// bit 1 of r: the neighbour differs from r in bits 1 .. l only, so it lies in the same aligned 2^(l+1) positions (co_prev),
// and the driver streams in aligned blocks of 2^(max(lp, lq) + 1) rows.
#pragma once
#include "k_commit.hpp"
#include "k_sample.hpp"

namespace rsv {

// Per proof: CO_PARAM_Q QM31 entries — rc^0 .. rc^85, z, alpha, alpha^2, plonk_sum / 2^lp, poseidon_sum / 2^lq.
constexpr uint32_t CO_POWERS = 86, CO_Z = 86, CO_ALPHA = 87, CO_ALPHA2 = 88, CO_SHIFT_P = 89, CO_SHIFT_Q = 90, CO_PARAM_Q = 92;
constexpr uint32_t CO_MAX_PARTS = 5;

// One lane per proof of the pass; draws [n][12] = z, alpha, random_coeff and sums [n][2][4]: any u32 is taken mod P.
__global__ __launch_bounds__(64) void k_co_params(const uint32_t* __restrict__ draws, const uint32_t* __restrict__ sums,
                                                  const uint8_t* __restrict__ mask, uint32_t p0, uint32_t n_pass, uint32_t lp, uint32_t lq,
                                                  uint32_t* __restrict__ par) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pass || (mask && !mask[p0 + p])) return;
    const uint32_t* d = draws + (uint64_t)(p0 + p) * 12;
    const uint32_t* s = sums + (uint64_t)(p0 + p) * 8;
    uint32_t* o = par + (uint64_t)p * CO_PARAM_Q * 4;
    auto put = [&](uint32_t e, QM31 v) {
        o[e * 4] = v.a.a;
        o[e * 4 + 1] = v.a.b;
        o[e * 4 + 2] = v.b.a;
        o[e * 4 + 3] = v.b.b;
    };
    const QM31 rc = sp_load_q(d + 8), alpha = sp_load_q(d + 4);
    QM31 w = q_one();
#pragma unroll 1
    for (uint32_t e = 0; e < CO_POWERS; e++) {
        put(e, w);
        w = q_mul(w, rc);
    }
    put(CO_Z, sp_load_q(d));
    put(CO_ALPHA, alpha);
    put(CO_ALPHA2, q_mul(alpha, alpha));
    put(CO_SHIFT_P, q_mul_m(sp_load_q(s), 1u << (31 - lp)));  // 2^-l = 2^(31-l) mod P (data_structures.rs:67-68)
    put(CO_SHIFT_Q, q_mul_m(sp_load_q(s + 4), 1u << (31 - lq)));
    put(CO_PARAM_Q - 1, q_zero());
}

// zinv[t] = 1 / Z_l at the positions r with r >> l == t of the domain 2^clb; 2^(clb - l) entries, one lane each.
__global__ __launch_bounds__(256) void k_co_zinv(uint32_t clb, uint32_t l, uint32_t* __restrict__ zinv) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)1 << (clb - l))) return;
    const uint64_t i = bit_reverse((uint32_t)t, clb - l);  // the low clb - l bits of the natural index
    const uint64_t idx = (((uint64_t)1 << (30 - clb)) + (i << (32 - clb))) << (l - 1);
    zinv[t] = m_inv(cp_gen_mul((uint32_t)(idx & 0x7fffffffu)).x);
}

// The extended columns of one component in a pass: column c (component order: preprocessed, trace, interaction) of proof
// p (of the pass) is in the part with the largest col0 <= c, at base + p * pstride + ((c - col0) << rlog) + row.
struct CoPart {
    const uint32_t* base;
    uint64_t pstride;  // 0: shared by every proof
    uint32_t col0;
};
struct CoRows {
    CoPart part[CO_MAX_PARTS];
    uint32_t n_parts;
    uint32_t log, rlog;     // the component's log size; 2^rlog rows per proof in this pass (an aligned block of the domain)
    uint64_t row0;          // the block's first position in the domain 2^clb
    const uint32_t* par;    // [proofs of the pass][CO_PARAM_Q][4]
    const uint32_t* zinv;   // k_co_zinv's table of this component
    const uint8_t* mask;    // a proof whose byte (index p0 + p) is 0 is skipped
    uint32_t p0, clb;
    uint32_t* acc;          // [proofs of the pass][4][2^clb]: k_co_plonk writes rc^80 A_plonk, k_co_poseidon adds A_poseidon
};

__device__ __forceinline__ uint32_t co_col(const CoRows& a, uint32_t p, uint32_t c, uint32_t r) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t i = 1; i < CO_MAX_PARTS; i++)
        if (i < a.n_parts && c >= a.part[i].col0) k = i;
    return a.part[k].base[p * a.part[k].pstride + ((uint64_t)(c - a.part[k].col0) << a.rlog) + r];
}
// The position of the previous row of a column of 2^l rows (header comment).
__device__ __forceinline__ uint32_t co_prev(uint32_t r, uint32_t l) {
    const uint32_t m = (2u << l) - 1, w = r & m, half = w & 1u;
    uint32_t j = bit_reverse(w >> 1, l);
    j = (half ? j + 1 : j - 1) & ((1u << l) - 1);
    return (r & ~m) | (bit_reverse(j, l) << 1) | half;
}
__device__ __forceinline__ QM31 co_ldq(const uint32_t* par, uint32_t e) { return q_mk(par[e * 4], par[e * 4 + 1], par[e * 4 + 2], par[e * 4 + 3]); }

// Unreduced sums of M31 constraint x rc^e, four words.  As next to sp_fold: a word holds a folded remainder < 2^34 plus
// at most four products of canonical words, 4 (2^31 - 2)^2 + 2^34 < 2^64; the callers fold after every fourth product
// (`fold`), and co_value folds once more before sp_canon.  Both operands are canonical: the constraint comes out of m_*
// arithmetic, the power out of k_co_params' q_mul.
struct CoAcc {
    uint64_t a[4] = {0, 0, 0, 0};
    __device__ __forceinline__ void add(const uint32_t* par, uint32_t e, uint32_t c, bool fold) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            a[j] += (uint64_t)c * par[e * 4 + j];
            if (fold) a[j] = sp_fold(a[j]);
        }
    }
    __device__ __forceinline__ QM31 value() const {
        return q_mk(sp_canon(sp_fold(a[0])), sp_canon(sp_fold(a[1])), sp_canon(sp_fold(a[2])), sp_canon(sp_fold(a[3])));
    }
};

// This lane's proof (of the pass) and row (of the block); false for a surplus lane or a masked proof.
__device__ __forceinline__ bool co_lane(const CoRows& a, uint32_t& p, uint32_t& r) {
    const uint32_t bpp = a.rlog > 8 ? 1u << (a.rlog - 8) : 1u;  // workgroups per proof: a wave's rows belong to one proof
    p = blockIdx.x / bpp;
    r = (blockIdx.x - p * bpp) * 256 + threadIdx.x;
    return r < (1u << a.rlog) && !(a.mask && !a.mask[a.p0 + p]);
}

// plonk.rs:8-82 on one row: columns 0..9 preprocessed, 10..21 trace, 22..29 interaction.
__global__ __launch_bounds__(256) void k_co_plonk(CoRows a) {
    uint32_t p, r;
    if (!co_lane(a, p, r)) return;
    const uint32_t* par = a.par + (uint64_t)p * CO_PARAM_Q * 4;
    auto col = [&](uint32_t c) { return co_col(a, p, c, r); };
    const uint32_t enforce = col(9), op = col(3), t9 = col(19), t10 = col(20), t11 = col(21);
    CoAcc m;
    m.add(par, 85, m_mul(enforce, t9), false);
    m.add(par, 84, m_mul(enforce, t10), false);
    m.add(par, 83, m_mul(enforce, t11), false);
    const QM31 A = q_mk(col(10), col(11), col(12), col(13)), B = q_mk(col(14), col(15), col(16), col(17)), C = q_mk(col(18), t9, t10, t11);
    const QM31 gate = q_sub(q_sub(C, q_mul_m(q_add(A, B), op)), q_mul(q_mul_m(A, m_sub(1u, op)), B));
    QM31 s = q_mul(gate, co_ldq(par, 82));
    const QM31 z = co_ldq(par, CO_Z), alpha = co_ldq(par, CO_ALPHA), alpha2 = co_ldq(par, CO_ALPHA2);
    const QM31 fq0 = q_sub(q_add(A, q_mul_m(alpha, col(0))), z), fq1 = q_sub(q_add(B, q_mul_m(alpha, col(1))), z);
    const QM31 fq2 = q_sub(q_add(C, q_mul_m(alpha, col(2))), z);
    const QM31 fq3 = q_sub(q_add(q_add(q_from_m(col(7)), q_mul(alpha, A)), q_mul(alpha2, B)), z);
    const uint32_t fp0 = col(4), fp1 = col(5), fp2 = col(6), fp3 = m_neg(col(8));
    // finalize_logup, batches of two: (0, 1) against columns 0..3, (2, 3) against the cumulative columns 4..7
    const QM31 cur0 = q_mk(col(22), col(23), col(24), col(25));
    s = q_add(s, q_mul(q_sub(q_mul(cur0, q_mul(fq0, fq1)), q_add(q_mul_m(fq1, fp0), q_mul_m(fq0, fp1))), co_ldq(par, 81)));
    const uint32_t rp = co_prev(r, a.log);
    const QM31 cur = q_mk(col(26), col(27), col(28), col(29));
    const QM31 prev = q_mk(co_col(a, p, 26, rp), co_col(a, p, 27, rp), co_col(a, p, 28, rp), co_col(a, p, 29, rp));
    const QM31 diff = q_add(q_sub(q_sub(cur, prev), cur0), co_ldq(par, CO_SHIFT_P));
    s = q_add(s, q_mul(q_sub(q_mul(diff, q_mul(fq2, fq3)), q_add(q_mul_m(fq3, fp2), q_mul_m(fq2, fp3))), co_ldq(par, 80)));
    const uint64_t at = a.row0 + r;
    const QM31 v = q_mul_m(q_add(m.value(), s), a.zinv[at >> a.log]);
    uint32_t* o = a.acc + (((uint64_t)p * 4) << a.clb) + at;
    o[0] = v.a.a;
    o[(uint64_t)1 << a.clb] = v.a.b;
    o[(uint64_t)2 << a.clb] = v.b.a;
    o[(uint64_t)3 << a.clb] = v.b.b;
}

// poseidon.rs:12-71 over M31
__device__ __forceinline__ void co_m4(uint32_t* x) {
    const uint32_t t0 = m_add(x[0], x[1]), t02 = m_dbl(t0), t1 = m_add(x[2], x[3]), t12 = m_dbl(t1);
    const uint32_t t2 = m_add(m_dbl(x[1]), t1), t3 = m_add(m_dbl(x[3]), t0);
    const uint32_t t4 = m_add(m_dbl(t12), t3), t5 = m_add(m_dbl(t02), t2);
    x[0] = m_add(t3, t5);
    x[1] = t5;
    x[2] = m_add(t2, t4);
    x[3] = t4;
}
__device__ __forceinline__ void co_external(uint32_t* s) {
#pragma unroll
    for (int g = 0; g < 4; g++) co_m4(s + 4 * g);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t sum = m_add(m_add(s[j], s[j + 4]), m_add(s[j + 8], s[j + 12]));
#pragma unroll
        for (int g = 0; g < 4; g++) s[4 * g + j] = m_add(s[4 * g + j], sum);
    }
}
__device__ __forceinline__ void co_internal(uint32_t* s) {
    uint32_t sum = s[0];
#pragma unroll
    for (int i = 1; i < 16; i++) sum = m_add(sum, s[i]);
    s[0] = m_add(s[0], m_add(m_dbl(s[0]), sum));
#pragma unroll
    for (int i = 1; i < 16; i++) s[i] = m_add(m_shl(s[i], i + 1), sum);
}
__device__ __forceinline__ uint32_t co_pow5(uint32_t x) {
    const uint32_t x2 = m_sqr(x);
    return m_mul(m_sqr(x2), x);
}

// poseidon.rs:73-241 on one row: columns 0..39 preprocessed, 40..87 trace (in, mid, out), 88..95 interaction.  Constraint
// j (0 .. 79) is weighted by rc^(79 - j); the first 78 are M31.
__global__ __launch_bounds__(256) void k_co_poseidon(CoRows a) {
    uint32_t p, r;
    if (!co_lane(a, p, r)) return;
    const uint32_t* par = a.par + (uint64_t)p * CO_PARAM_Q * 4;
    auto col = [&](uint32_t c) { return co_col(a, p, c, r); };
    const uint32_t is_first = col(0), is_last = col(1), is_full = col(2), round_id = col(3);
    const uint32_t not_first = m_sub(1u, is_first), not_last = m_sub(1u, is_last), is_partial = m_sub(not_first, is_full);
    uint32_t in[16], mid[16], out[16], st[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        in[i] = col(40 + i);
        mid[i] = col(56 + i);
        out[i] = col(72 + i);
    }
    CoAcc m;
    uint32_t j = 0;  // the constraint's index: a constant after unrolling
    const uint32_t swap = mid[0], keep = m_sub(1u, swap);
#pragma unroll
    for (int i = 0; i < 16; i++) st[i] = m_add(m_mul(in[i], keep), m_mul(in[i ^ 8], swap));
    co_external(st);
#pragma unroll
    for (int i = 0; i < 16; i++, j++) m.add(par, 79 - j, m_mul(is_first, m_sub(st[i], out[i])), (j & 3) == 3);
    // full round
#pragma unroll
    for (int i = 0; i < 16; i++, j++) {
        m.add(par, 79 - j, m_mul(is_full, m_sub(mid[i], co_pow5(m_add(in[i], col(4 + i))))), (j & 3) == 3);
        st[i] = mid[i];
    }
    co_external(st);
#pragma unroll
    for (int i = 0; i < 16; i++) st[i] = co_pow5(m_add(st[i], col(20 + i)));
    co_external(st);
#pragma unroll
    for (int i = 0; i < 16; i++, j++) m.add(par, 79 - j, m_mul(is_full, m_sub(out[i], st[i])), (j & 3) == 3);
    // partial rounds
#pragma unroll
    for (int i = 0; i < 16; i++) st[i] = in[i];
#pragma unroll
    for (int k = 0; k < 14; k++, j++) {
        m.add(par, 79 - j, m_mul(is_partial, m_sub(mid[k], co_pow5(m_add(st[0], col(4 + k))))), (j & 3) == 3);
        st[0] = mid[k];
        co_internal(st);
    }
#pragma unroll
    for (int i = 0; i < 16; i++, j++) m.add(par, 79 - j, m_mul(is_partial, m_sub(out[i], st[i])), (j & 3) == 3);
    // lookups: five fractions in batches of three, (0, 1, 2) against columns 0..3, (3, 4) against the cumulative 4..7
    const QM31 z = co_ldq(par, CO_Z), alpha = co_ldq(par, CO_ALPHA), alpha2 = co_ldq(par, CO_ALPHA2);
    const uint32_t ext1 = col(36), ext2 = col(37), ext1_nz = col(38), ext2_nz = col(39);
    const uint32_t in_left = m_dbl(round_id), in_right = m_add(in_left, 1u), out_left = m_add(in_right, 1u), out_right = m_add(out_left, 1u);
    auto rel3 = [&](uint32_t v0, const uint32_t* w) {
        return q_sub(q_add(q_add(q_from_m(v0), q_mul(alpha, q_mk(w[0], w[1], w[2], w[3]))), q_mul(alpha2, q_mk(w[4], w[5], w[6], w[7]))), z);
    };
    const QM31 fq0 = rel3(m_add(m_mul(is_first, ext1), m_mul(not_first, in_left)), in);
    const QM31 fq1 = rel3(m_add(m_mul(is_first, ext2), m_mul(not_first, in_right)), in + 8);
    const QM31 fq2 = rel3(m_add(m_mul(is_last, ext1), m_mul(not_last, out_left)), out);
    const QM31 fq3 = rel3(m_add(m_mul(is_last, ext2), m_mul(not_last, out_right)), out + 8);
    const QM31 fq4 = q_sub(q_add(q_from_m(swap), q_mul_m(alpha, col(4))), z);
    const uint32_t fp0 = m_sub(m_mul(ext1_nz, is_first), not_first), fp1 = m_sub(m_mul(ext2_nz, is_first), not_first);
    const uint32_t fp2 = m_add(m_mul(ext1_nz, is_last), not_last), fp3 = m_add(m_mul(ext2_nz, is_last), not_last);
    const uint32_t fp4 = m_mul(is_first, not_last);
    const QM31 q01 = q_mul(fq0, fq1);
    const QM31 pp0 = q_add(q_mul(q_add(q_mul_m(fq1, fp0), q_mul_m(fq0, fp1)), fq2), q_mul_m(q01, fp2));
    const QM31 cur0 = q_mk(col(88), col(89), col(90), col(91));
    QM31 s = q_mul(q_sub(q_mul(cur0, q_mul(q01, fq2)), pp0), co_ldq(par, 1));
    const uint32_t rp = co_prev(r, a.log);
    const QM31 cur = q_mk(col(92), col(93), col(94), col(95));
    const QM31 prev = q_mk(co_col(a, p, 92, rp), co_col(a, p, 93, rp), co_col(a, p, 94, rp), co_col(a, p, 95, rp));
    const QM31 diff = q_add(q_sub(q_sub(cur, prev), cur0), co_ldq(par, CO_SHIFT_Q));
    s = q_add(s, q_sub(q_mul(diff, q_mul(fq3, fq4)), q_add(q_mul_m(fq4, fp3), q_mul_m(fq3, fp4))));  // times rc^0
    const uint64_t at = a.row0 + r;
    const QM31 v = q_mul_m(q_add(m.value(), s), a.zinv[at >> a.log]);
    uint32_t* o = a.acc + (((uint64_t)p * 4) << a.clb) + at;
    o[0] = m_add(o[0], v.a.a);
    o[(uint64_t)1 << a.clb] = m_add(o[(uint64_t)1 << a.clb], v.a.b);
    o[(uint64_t)2 << a.clb] = m_add(o[(uint64_t)2 << a.clb], v.b.a);
    o[(uint64_t)3 << a.clb] = m_add(o[(uint64_t)3 << a.clb], v.b.b);
}

// The cut at the middle: the coefficients coef [P][4][2^(L3+1)] of the four coordinates -> out [P][8][2^L3], column k the
// low half (left) of coordinate k, column 4 + k its high half (right).  One lane per word.
__global__ __launch_bounds__(256) void k_co_cut(const uint32_t* __restrict__ coef, uint32_t L3, uint32_t n_pass, uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)n_pass * 8) << L3) return;
    const uint64_t i = t & (((uint64_t)1 << L3) - 1), pc = t >> L3;
    const uint32_t c = (uint32_t)(pc & 7);
    out[t] = coef[((((pc >> 3) * 4 + (c & 3)) * 2 + (c >> 2)) << L3) + i];
}

// The next transcript after random_coeff, one lane per proof (run_transcript order): mix root 3, draw t, the OODS point
// ((1 - t^2) / (1 + t^2), 2 t / (1 + t^2)) (CirclePointQM31Var::from_t).  chan [n][16] as k_cm_draw_coeff leaves it, read
// and updated; oods [n][8]: x then y.  A proof with ok == 0 gets zeros in both.
__global__ __launch_bounds__(64) void k_co_draw_oods(const uint32_t* __restrict__ root3, const uint8_t* __restrict__ ok_in, uint32_t n,
                                                     uint32_t* __restrict__ chan, uint32_t* __restrict__ oods) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    uint32_t* co = chan + (size_t)p * 16;
    uint32_t* o = oods + (size_t)p * 8;
    if (ok_in && !ok_in[p]) {
#pragma unroll
        for (int i = 0; i < 16; i++) co[i] = 0u;
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = 0u;
        return;
    }
    Channel<0> ch = channel_load(co);
    ch.mix(load_hash(root3 + (size_t)p * 8));
    const QM31 t = q_lo(ch.draw());
    const QM31 t2 = q_mul(t, t), inv = q_inv(q_add(t2, q_one()));
    const QM31 x = q_mul(q_sub(q_one(), t2), inv), y = q_mul(q_dbl(t), inv);
    channel_store(co, ch);
    o[0] = x.a.a; o[1] = x.a.b; o[2] = x.b.a; o[3] = x.b.b;
    o[4] = y.a.a; o[5] = y.a.b; o[6] = y.b.a; o[7] = y.b.b;
}

}  // namespace rsv
