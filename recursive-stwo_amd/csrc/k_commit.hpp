// k_commit.hpp — commitment of a tree of the next proof: circle interpolation, low-degree extension (LDE) and stwo's
// mixed-size Merkle tree (commit_api.inc drives the launches; include/rsv.h: rsv_commit_tree_dev).
//
// Bit-reversed storage of a circle domain of size 2^N (CanonicCoset(N).circle_domain(), as k_trace / k_interaction store
// their columns): butterfly layer m pairs positions p and p + 2^m (bit m of p clear).  Its twiddle is, for layer 0, the y
// and, for layer m >= 1, the x of 2^(m-1) * half_coset.at(bitrev_(N-1)((p >> (m + 1)) << m)), half_coset =
// Coset::half_odds(N - 1).  The inverse layers 0, 1, ..., N-1 (then a factor 2^-N) give the CirclePoly coefficients in
// natural order (coefficient i multiplies y^{i_0} x^{i_1} pi(x)^{i_2} ...); the forward layers N-1, ..., 0 on the
// zero-padded coefficients give the evaluation on a larger domain.  With coefficients beyond 2^log zero, the layers
// m >= log of the domain 2^(log+b) only copy, so its block k = positions [k 2^log, (k+1) 2^log) is the forward FFT of
// the coefficients with layers log-1 .. 0, twiddled at the block's absolute positions: the LDE streams block by block.
// The Merkle subtree of block k covers the same block of every smaller column and ends in one node at layer b.
#pragma once
#include "circle.hpp"
#include "merkle.hpp"

namespace rsv {

constexpr uint32_t CM_MAX_GROUPS = 8;  // RSV_MAX_COMMIT_GROUPS
constexpr uint32_t CM_LDS_LOG = 12;    // butterfly layers 0..11 of a 4 096-point chunk run in LDS, the layers above in global passes

// Twiddle table of the domain 2^N: layer m (0 <= m < N) at offset 2^N - 2^(N-m), 2^(N-1-m) entries; 2^N - 1 words.
__host__ __device__ __forceinline__ uint64_t cm_tw_off(uint32_t N, uint32_t m) { return ((uint64_t)1 << N) - ((uint64_t)1 << (N - m)); }

__global__ __launch_bounds__(256) void k_cm_twiddles(uint32_t* __restrict__ tw, uint32_t N, uint32_t inverse) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)1 << N) - 1) return;
    uint32_t m = 0;
    while (t >= cm_tw_off(N, m + 1)) m++;
    const uint32_t k = (uint32_t)(t - cm_tw_off(N, m));
    const uint32_t br = N > 1 ? bit_reverse(k << m, N - 1) : 0u;
    // half_coset.at(i) = (2^(30-N) + i 2^(32-N)) * GEN, indices mod 2^31
    uint64_t idx = ((uint64_t)1 << (30 - N)) + ((uint64_t)br << (32 - N));
    if (m) idx <<= (m - 1);
    const CPoint pt = cp_gen_mul((uint32_t)(idx & 0x7fffffffu));
    const uint32_t v = m ? pt.x : pt.y;
    tw[t] = inverse ? m_inv(v) : v;
}

// A set of rows of 2^log words: row (pc, kb) at base + pc * pc_stride + kb * 2^log, pc = proof * n_cols + column, kb < nb
// a block of the domain 2^N at absolute block index blk0 + kb (twiddle positions).
struct CmRows {
    uint32_t* base;
    uint64_t pc_stride;
    uint64_t rows;  // (#pc) * nb
    uint32_t log, N, nb, blk0;
};
// Where a row's first layer reads from (base == nullptr: the row itself): proof pc / cols, column pc % cols at
// base + proof * pstride + column * cstride; a proof whose mask byte (index p0 + proof) is 0 reads zeros; values times scale.
struct CmSrc {
    const uint32_t* base;
    uint64_t pstride, cstride;
    const uint8_t* mask;
    uint32_t cols, p0, scale;
};

__device__ __forceinline__ uint32_t* cm_row(const CmRows& r, uint64_t row, uint32_t& kb) {
    const uint64_t pc = row / r.nb;
    kb = (uint32_t)(row - pc * r.nb);
    return r.base + pc * r.pc_stride + ((uint64_t)kb << r.log);
}
__device__ __forceinline__ const uint32_t* cm_src(const CmSrc& s, uint64_t pc, uint32_t& scale) {
    const uint64_t p = pc / s.cols, c = pc - p * s.cols;
    scale = (s.mask && !s.mask[s.p0 + p]) ? 0u : s.scale;
    return s.base + p * s.pstride + c * s.cstride;
}
template <bool INV>
__device__ __forceinline__ void cm_butterfly(uint32_t& a, uint32_t& b, uint32_t w) {
    if (INV) {
        const uint32_t s = m_add(a, b);
        b = m_mul(m_sub(a, b), w);
        a = s;
    } else {
        const uint32_t t = m_mul(b, w);
        b = m_sub(a, t);
        a = m_add(a, t);
    }
}

// One butterfly layer m >= CM_LDS_LOG over every row of the set, one lane per pair.
template <bool INV>
__global__ __launch_bounds__(256) void k_cm_fft_layer(CmRows r, CmSrc s, const uint32_t* __restrict__ tw, uint32_t m) {
    const uint32_t hl = r.log - 1;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (r.rows << hl)) return;
    const uint64_t row = t >> hl;
    const uint32_t j = (uint32_t)(t & ((1u << hl) - 1));
    const uint32_t p = ((j >> m) << (m + 1)) | (j & ((1u << m) - 1)), q = p + (1u << m);
    uint32_t kb;
    uint32_t* d = cm_row(r, row, kb);
    uint32_t a, b;
    if (s.base) {
        uint32_t sc;
        const uint32_t* src = cm_src(s, row / r.nb, sc);
        a = m_mul(src[p], sc);
        b = m_mul(src[q], sc);
    } else {
        a = d[p];
        b = d[q];
    }
    cm_butterfly<INV>(a, b, tw[cm_tw_off(r.N, m) + ((((uint64_t)(r.blk0 + kb) << r.log) + p) >> (m + 1))]);
    d[p] = a;
    d[q] = b;
}

// The butterfly layers 0 .. c-1 (inverse: ascending, forward: descending) of 2^c-point chunks in LDS, one workgroup per
// chunk; 2^(log - c) chunks per row.
template <bool INV>
__global__ __launch_bounds__(256) void k_cm_fft_lds(CmRows r, CmSrc s, const uint32_t* __restrict__ tw, uint32_t c) {
    __shared__ uint32_t v[1u << CM_LDS_LOG];
    const uint32_t C = 1u << c, per_row_log = r.log - c;
    const uint64_t row = (uint64_t)blockIdx.x >> per_row_log;
    const uint32_t ch = blockIdx.x & ((1u << per_row_log) - 1);
    uint32_t kb;
    uint32_t* d = cm_row(r, row, kb) + (uint64_t)ch * C;
    if (s.base) {
        uint32_t sc;
        const uint32_t* src = cm_src(s, row / r.nb, sc) + (uint64_t)ch * C;
        for (uint32_t i = threadIdx.x; i < C; i += 256) v[i] = m_mul(src[i], sc);
    } else {
        for (uint32_t i = threadIdx.x; i < C; i += 256) v[i] = d[i];
    }
    __syncthreads();
    const uint64_t abs0 = ((uint64_t)(r.blk0 + kb) << r.log) + (uint64_t)ch * C;
    for (uint32_t k = 0; k < c; k++) {
        const uint32_t m = INV ? k : c - 1 - k;
        const uint32_t* twm = tw + cm_tw_off(r.N, m);
        for (uint32_t j = threadIdx.x; j < C / 2; j += 256) {
            const uint32_t p = ((j >> m) << (m + 1)) | (j & ((1u << m) - 1)), q = p + (1u << m);
            uint32_t a = v[p], b = v[q];
            cm_butterfly<INV>(a, b, twm[(abs0 + p) >> (m + 1)]);
            v[p] = a;
            v[q] = b;
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < C; i += 256) d[i] = v[i];
}

// ---------------------------------------------------------------- Merkle
// The columns of one group at a layer: proof p, column c, block kb, node j at base + (p n_cols + c) pc_stride + kb 2^lw + j.
struct CmLayerCols {
    const uint32_t* base;
    uint64_t pc_stride;
    uint32_t n_cols;
};
struct CmHashArgs {
    CmLayerCols g[CM_MAX_GROUPS];  // the groups whose LDE lives at this layer, in commitment order
    uint32_t ng, n_cols;           // their number, their columns in all
    uint32_t lw, nb, P;            // 2^lw nodes per block at this layer, nb blocks, P proofs
    const uint32_t* child;         // the layer above: [P][nb][2^(lw+1)][8], nullptr at the leaves
    uint32_t* out;                 // [P][nb][2^lw][8]; at lw == 0 (the block roots) [P][2^b][8] at block blk0 + kb
    uint32_t blk0, b;
};

// hash_node(children, columns) of every node of a layer of the block subtrees, one lane per node.
__global__ __launch_bounds__(256) void k_cm_hash_layer(CmHashArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)a.P * a.nb << a.lw)) return;
    const uint32_t j = (uint32_t)(t & ((1u << a.lw) - 1));
    const uint64_t rest = t >> a.lw;
    const uint32_t p = (uint32_t)(rest / a.nb), kb = (uint32_t)(rest - (uint64_t)p * a.nb);
    const uint64_t at = ((uint64_t)kb << a.lw) + j;
    Hash8 d = zero8();
    uint32_t gi = 0, ci = 0;
    for (uint32_t off = 0; off < a.n_cols; off += 8) {
        Hash8 chunk;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            uint32_t w = 0;
            if (off + k < a.n_cols) {
                const CmLayerCols& g = a.g[gi];
                w = g.base[((uint64_t)p * g.n_cols + ci) * g.pc_stride + at];
                if (++ci == g.n_cols) { ci = 0; gi++; }
            }
            chunk.w[k] = w;
        }
        d = perm_cap<1>(chunk, d);
    }
    Hash8 h;
    if (!a.child) {
        h = leaf_from_capacity<1>(d);
    } else {
        const uint32_t* cp = a.child + (t << 1) * 8;
        const Hash8 l = load_hash(cp), r = load_hash(cp + 8);
        h = hash_tree<1>(l, r);
        if (a.n_cols) h = combine_with_column<1>(h, d);
    }
    uint32_t* o = a.lw ? a.out + t * 8 : a.out + (((uint64_t)p << a.b) + a.blk0 + kb) * 8;
    store_hash(o, h);
}

// A plain node layer above the block roots: in [P][2^(l+1)][8] -> out [P][2^l][8]; at l == 0 the root of proof p goes to
// roots + (p0 + p) * roots_stride, zero where mask[p0 + p] == 0.
__global__ __launch_bounds__(256) void k_cm_top(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t l, uint32_t P,
                                                uint32_t* __restrict__ roots, uint32_t roots_stride, const uint8_t* __restrict__ mask,
                                                uint32_t p0) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)P << l)) return;
    const Hash8 h = hash_tree<1>(load_hash(in + t * 16), load_hash(in + t * 16 + 8));
    if (l) {
        store_hash(out + t * 8, h);
        return;
    }
    const bool keep = !mask || mask[p0 + t];
    uint32_t* o = roots + (uint64_t)(p0 + t) * roots_stride;
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = keep ? h.w[i] : 0u;
}

// ---------------------------------------------------------------- the recursion circuit's chain (rsv_witness_commit_dev)
// Tree 0's op column of every proof: the template's, with the witness-dependent rows from d_ops ([n][n_ops]).
__global__ __launch_bounds__(256) void k_cm_op_column(const uint32_t* __restrict__ tmpl, uint32_t log, uint32_t n, uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)n << log)) return;
    out[t] = tmpl[t & ((1u << log) - 1)];
}
__global__ __launch_bounds__(256) void k_cm_op_patch(const uint32_t* __restrict__ wops, uint32_t n_ops, const uint32_t* __restrict__ ops,
                                                     uint32_t log, uint32_t n, uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n_ops * n) return;
    const uint64_t p = t / n_ops, k = t - p * n_ops;
    out[(p << log) + wops[3 * k]] = ops[t];
}

// The next transcript's prefix, one lane per proof (run_transcript order): mix root 0, lp, lq, root 1, draw (z, alpha).
// chan [n][16]: digest[8], n_sent, 7 zero words.
__global__ __launch_bounds__(64) void k_cm_draw_lookup(const uint32_t* __restrict__ roots, uint32_t lp, uint32_t lq, uint32_t n,
                                                       uint32_t* __restrict__ lookup, uint32_t* __restrict__ chan) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    Channel<0> ch;
    ch.init();
    ch.mix(load_hash(roots + (size_t)p * 24));
    ch.mix_one(q_from_m(lp));
    ch.mix_one(q_from_m(lq));
    ch.mix(load_hash(roots + (size_t)p * 24 + 8));
    store_hash(lookup + (size_t)p * 8, ch.draw());
    store_hash(chan + (size_t)p * 16, ch.digest);
    chan[(size_t)p * 16 + 8] = ch.n_sent;
}
// ... then mix the two claimed sums and root 2, draw random_coeff; every output of a proof with ok == 0 is zeroed.
__global__ __launch_bounds__(64) void k_cm_draw_coeff(uint32_t* __restrict__ roots, const uint32_t* __restrict__ lookup,
                                                      const uint32_t* __restrict__ sums, const uint8_t* __restrict__ ok_in, uint32_t n,
                                                      uint32_t* __restrict__ chan, uint32_t* __restrict__ draws,
                                                      uint32_t* __restrict__ chan_out, uint8_t* __restrict__ ok_out) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    Channel<0> ch = channel_load(chan + (size_t)p * 16);
    Hash8 s = load_hash(sums + (size_t)p * 8);
    ch.mix(s);
    ch.mix(load_hash(roots + (size_t)p * 24 + 16));
    const Hash8 rc = ch.draw();
    const bool ok = ok_in[p] != 0;
    const Hash8 lk = load_hash(lookup + (size_t)p * 8);
    uint32_t* dr = draws + (size_t)p * 12;
#pragma unroll
    for (int i = 0; i < 8; i++) dr[i] = ok ? lk.w[i] : 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) dr[8 + i] = ok ? rc.w[i] : 0u;
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 24; i++) roots[(size_t)p * 24 + i] = 0u;
    }
    if (chan_out) {
        uint32_t* co = chan_out + (size_t)p * 16;
#pragma unroll
        for (int i = 0; i < 8; i++) co[i] = ok ? ch.digest.w[i] : 0u;
        co[8] = ok ? ch.n_sent : 0u;
#pragma unroll
        for (int i = 9; i < 16; i++) co[i] = 0u;
    }
    if (ok_out) ok_out[p] = ok ? 1 : 0;
}

}  // namespace rsv
