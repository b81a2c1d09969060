// k_sample.hpp — the sampled values of committed columns: CirclePoly::eval_at_point of every column at up to four QM31
// points per proof (sample_api.inc drives the launches; include/rsv.h: rsv_sample_tree_dev).
//
// For coefficients c_i in k_commit.hpp's order (coefficient i multiplies y^{i_0} x^{i_1} pi(x)^{i_2} ..., i_k = bit k of i)
// the value at (x, y) is sum_i c_i prod_k f_k^{i_k} with f_0 = y, f_1 = x, f_{k+1} = 2 f_k^2 - 1 in QM31: a dot product
// of M31 coefficients with QM31 weights.  The index is split i = (hi, lo), lo = the low SP_LANE_LOG = 8 bits, and the
// weight with it, W_i = W_hi W_lo: a lane owns lo (consecutive lanes read consecutive words), walks hi with the
// wave-uniform W_hi as a scalar operand — four M31 x M31 multiply-accumulates per coefficient and point — and multiplies
// its QM31 sum once by its own W_lo.  A workgroup covers a chunk of 2^SP_CHUNK_LOG coefficients of one column and leaves
// one QM31 per point; k_sp_finish adds a column's chunks and places the value.  Each coefficient is read once for all
// points of its column.  k_sp_weights writes the tables, one per (proof, point, domain size).
#pragma once
#include "circle.hpp"

namespace rsv {

constexpr uint32_t SP_LANE_LOG = 8;    // index bits 0..7: the lane
constexpr uint32_t SP_CHUNK_LOG = 13;  // coefficients per workgroup: columns above 2^13 rows are cut into 2^(log - 13) chunks
constexpr uint32_t SP_MAX_POINTS = 4;  // RSV_MAX_SAMPLE_POINTS

// Entries of a weight table: 256 W_lo, then 2^max(log - 8, 0) W_hi; four words each.
__host__ __device__ __forceinline__ uint64_t sp_table_entries(uint32_t log) {
    return 256u + ((uint64_t)1 << (log > SP_LANE_LOG ? log - SP_LANE_LOG : 0));
}

__device__ __forceinline__ uint32_t sp_mod_p(uint32_t w) {  // any u32 mod P
    const uint32_t s = (w & P) + (w >> 31);
    return min(s, s - P);
}
__device__ __forceinline__ QM31 sp_load_q(const uint32_t* p) { return q_mk(sp_mod_p(p[0]), sp_mod_p(p[1]), sp_mod_p(p[2]), sp_mod_p(p[3])); }

// The points of one launch: proof p's point k at pts + (p * np_in + k) * 8, x then y, any u32 words.  With prev_log != 0
// (np_in == 1, two tables per proof): table 0 is for the point minus the step of CanonicCoset(prev_log), the previous-row
// point of a column of that size, table 1 for the point itself.
struct SpPoints {
    const uint32_t* pts;
    uint32_t np_in, prev_log;
};

// wt [n_pass][np][sp_table_entries(log)][4] for the proofs p0 .. p0 + n_pass - 1 of a pass; one lane per entry.
__global__ __launch_bounds__(256) void k_sp_weights(SpPoints sp, uint32_t np, uint32_t log, uint32_t p0, uint32_t n_pass, uint32_t* __restrict__ wt) {
    const uint64_t entries = sp_table_entries(log);
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n_pass * np * entries) return;
    const uint64_t pk = t / entries, e = t - pk * entries;
    const uint32_t p = (uint32_t)(pk / np), k = (uint32_t)(pk - (uint64_t)p * np);
    const uint32_t* src = sp.pts + ((uint64_t)(p0 + p) * sp.np_in + (sp.prev_log ? 0 : k)) * 8;
    QM31 x = sp_load_q(src), y = sp_load_q(src + 4);
    if (sp.prev_log && k == 0) {
        // (x, y) - step: the step is GEN 2^(31 - prev_log), its inverse (sx, -sy)
        const uint32_t sx = GEN_POW.x[31 - sp.prev_log], sy = GEN_POW.y[31 - sp.prev_log];
        const QM31 nx = q_add(q_mul_m(x, sx), q_mul_m(y, sy));
        y = q_sub(q_mul_m(y, sx), q_mul_m(x, sy));
        x = nx;
    }
    // W_lo: the factors of bits 0..7 of e; W_hi: those of bits 8.. of (e - 256) << 8
    const uint64_t bits = e < 256 ? e : (e - 256) << SP_LANE_LOG;
    const uint32_t top = e < 256 ? SP_LANE_LOG : log;
    QM31 f = y, w = q_one();
    for (uint32_t b = 0; b < top; b++) {
        if ((bits >> b) & 1) w = q_mul(w, f);
        f = b == 0 ? x : q_sub(q_dbl(q_mul(f, f)), q_one());
    }
    uint32_t* o = wt + t * 4;
    o[0] = w.a.a;
    o[1] = w.a.b;
    o[2] = w.b.a;
    o[3] = w.b.b;
}

// The coefficients of one group in one pass: proof p (of the pass), column c at base + p * pstride + c * cstride, 2^log
// words; a proof whose mask byte (index p0 + p) is 0 is skipped (k_sp_finish writes its zeros).
struct SpCols {
    const uint32_t* base;
    uint64_t pstride, cstride;
    const uint8_t* mask;
    uint32_t p0, cols, log;
};

// Unreduced accumulation.  A sum word is a u64 that holds a folded remainder < 2^34 plus at most four products of a
// coefficient and a weight word, both <= P - 1 = 2^31 - 2: 4 (2^31 - 2)^2 + 2^34 = 2^64 - 2^35 + 2^34 + 16 < 2^64.  The
// fold x -> (x & P) + (x >> 31) keeps the residue and leaves < 2^31 + 2^33 < 2^34.  The coefficients are canonical words
// (the commitment's d_coeffs, the interpolation's output), the weights k_sp_weights' canonical products.  A caller's
// RSV_SAMPLE_COEFFS buffer with a word >= P is outside this bound: the sum may wrap and the value is then wrong, silently
// (include/rsv.h says so); nothing is read or written out of place.
__device__ __forceinline__ uint64_t sp_fold(uint64_t a) { return (a & P) + (a >> 31); }
__device__ __forceinline__ uint32_t sp_canon(uint64_t a) {  // a < 2^34 after sp_fold -> canonical
    const uint32_t s = (uint32_t)sp_fold(a);                // < 2^31 + 8
    return min(s, s - P);
}

// part [proofs of the pass * cols][NP][chunks][4]: the sum over a chunk of c_i W_i, canonical, per point.
template <uint32_t NP>
__global__ __launch_bounds__(256) void k_sp_dot(SpCols s, const uint32_t* __restrict__ wt, uint32_t* __restrict__ part) {
    __shared__ uint32_t red[4][NP][4];
    const uint32_t clog = s.log > SP_CHUNK_LOG ? s.log - SP_CHUNK_LOG : 0;
    const uint32_t chunk = blockIdx.x & ((1u << clog) - 1);
    const uint64_t pc = (uint64_t)blockIdx.x >> clog;
    const uint32_t p = (uint32_t)(pc / s.cols), col = (uint32_t)(pc - (uint64_t)p * s.cols);
    if (s.mask && !s.mask[s.p0 + p]) return;
    const uint32_t t = threadIdx.x;
    const uint32_t H = s.log > SP_LANE_LOG ? 1u << (min(s.log, SP_CHUNK_LOG) - SP_LANE_LOG) : 1u;  // hi steps of this chunk: 1 .. 32
    const uint64_t entries = sp_table_entries(s.log);
    const uint32_t* src = s.base + p * s.pstride + col * s.cstride + ((uint64_t)chunk << SP_CHUNK_LOG) + t;
    const uint32_t* w0 = wt + (uint64_t)p * NP * entries * 4;      // point k's table at w0 + k * entries * 4
    const uint32_t* whi = w0 + (256 + (uint64_t)chunk * H) * 4;    // this chunk's W_hi (chunk > 0 only where H == 32)
    uint64_t acc[NP][4] = {};
    if (H >= 4) {
        for (uint32_t h = 0; h < H; h += 4) {
            uint32_t c[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) c[u] = src[(h + u) << SP_LANE_LOG];
#pragma unroll
            for (uint32_t k = 0; k < NP; k++) {
                const uint32_t* w = whi + k * entries * 4 + h * 4;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    uint64_t a = acc[k][j];
#pragma unroll
                    for (uint32_t u = 0; u < 4; u++) a += (uint64_t)c[u] * w[u * 4 + j];
                    acc[k][j] = sp_fold(a);
                }
            }
        }
    } else {
        const bool live = s.log >= SP_LANE_LOG || t < (1u << s.log);
        for (uint32_t h = 0; h < H; h++) {  // at most two products per word
            const uint32_t c = live ? src[h << SP_LANE_LOG] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < NP; k++)
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) acc[k][j] += (uint64_t)c * whi[k * entries * 4 + h * 4 + j];
        }
#pragma unroll
        for (uint32_t k = 0; k < NP; k++)
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) acc[k][j] = sp_fold(acc[k][j]);
    }
    const uint32_t lane = t & 63, wave = t >> 6;
#pragma unroll
    for (uint32_t k = 0; k < NP; k++) {
        const uint32_t* wl = w0 + k * entries * 4 + t * 4;
        QM31 v = q_mul(q_mk(sp_canon(acc[k][0]), sp_canon(acc[k][1]), sp_canon(acc[k][2]), sp_canon(acc[k][3])), q_mk(wl[0], wl[1], wl[2], wl[3]));
#pragma unroll
        for (uint32_t d = 32; d >= 1; d >>= 1)
            v = q_add(v, q_mk(__shfl_xor(v.a.a, d), __shfl_xor(v.a.b, d), __shfl_xor(v.b.a, d), __shfl_xor(v.b.b, d)));
        if (lane == 0) {
            red[wave][k][0] = v.a.a;
            red[wave][k][1] = v.a.b;
            red[wave][k][2] = v.b.a;
            red[wave][k][3] = v.b.b;
        }
    }
    __syncthreads();
    if (t < NP * 4) {
        const uint32_t k = t >> 2, j = t & 3;
        const uint32_t v = m_add(m_add(red[0][k][j], red[1][k][j]), m_add(red[2][k][j], red[3][k][j]));
        part[(((pc * NP + k) << clog) + chunk) * 4 + j] = v;
    }
}

// Where a group's values go: proof p's at out + p * pstride (words).  Point-major (chain == 0): column c at point k at
// entry k * total_cols + col0 + c.  The proof's own order (chain == 1, column-major, sample-minor): the first `single`
// columns of the group have one value, at the LAST point, the others np values: entry col0 + c (c < single) or col0 +
// single + (c - single) * np + k.  Four words per entry.
struct SpOut {
    uint32_t* out;
    uint64_t pstride;
    uint32_t col0, total_cols, single, chain;
};

// The sum of a column's chunk sums, one lane per (proof, column, point); zeros for a masked proof.
__global__ __launch_bounds__(256) void k_sp_finish(const uint32_t* __restrict__ part, uint32_t np, uint32_t cols, uint32_t log, uint32_t n_pass,
                                                   const uint8_t* __restrict__ mask, uint32_t p0, SpOut o) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n_pass * cols * np) return;
    const uint64_t pc = t / np;
    const uint32_t k = (uint32_t)(t - pc * np);
    const uint32_t p = (uint32_t)(pc / cols), c = (uint32_t)(pc - (uint64_t)p * cols);
    uint64_t entry;
    if (!o.chain) entry = (uint64_t)k * o.total_cols + o.col0 + c;
    else if (c < o.single) {
        if (k + 1 != np) return;
        entry = o.col0 + c;
    } else entry = o.col0 + o.single + (uint64_t)(c - o.single) * np + k;
    QM31 v = q_zero();
    if (!mask || mask[p0 + p]) {
        const uint32_t chunks = 1u << (log > SP_CHUNK_LOG ? log - SP_CHUNK_LOG : 0);
        const uint32_t* q = part + t * chunks * 4;
        for (uint32_t i = 0; i < chunks; i++) v = q_add(v, q_mk(q[i * 4], q[i * 4 + 1], q[i * 4 + 2], q[i * 4 + 3]));
    }
    uint32_t* d = o.out + (uint64_t)(p0 + p) * o.pstride + entry * 4;
    d[0] = v.a.a;
    d[1] = v.a.b;
    d[2] = v.b.a;
    d[3] = v.b.b;
}

}  // namespace rsv
