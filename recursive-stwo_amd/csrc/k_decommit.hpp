// k_decommit.hpp — the opening of a streamed tree (decommit_api.inc drives the launches; include/rsv.h:
// rsv_decommit_tree_dev): the plan of a proof's queries, the block-list forms of the commitment's kernels, the cap levels
// and the gather of the planned words.
//
// stwo's batched decommitment (MerkleProver::decommit, consumed by SinglePathMerkleProof::from_stwo_proof) walks the tree
// from the largest layer `top` down.  At a layer the queried nodes are the distinct positions (queries >> (top - layer)) in
// ascending order; each carries that layer's column values, and for every distinct parent the child that is not itself
// queried is a witness node.  So both lists are runs per layer: the plan counts them (prefix sums over the layers give the
// slots) and names the nodes, the gather copies them where a pass has them:
//   values         from the LDE rows of the block (position >> (layer - b)) the node lies in,
//   witness > b    from the node layer of that block's subtree, right after k_cm_hash_layer made it,
//   witness <= b   from the cap: the nodes of layers 0 .. b in heap order (layer l at entries 2^l .. 2^(l+1) - 1).
#pragma once
#include "k_commit.hpp"

namespace rsv {

constexpr uint32_t DC_LAYERS = 32;  // layer tables of the plan: top <= RSV_MAX_LOG_SIZE = 30

// The plan of every proof (workspace).  Layer tables are [n][DC_LAYERS]; node tables [n][top + 1][nq]; witness tables
// [n][wcap], in output order.
struct DcPlan {
    uint32_t* cnt;     // [n] blocks in the proof's list (0: masked)
    uint32_t* blocks;  // [n][maxb] absolute block indices, ascending
    uint32_t* nl;      // distinct queried nodes of layer l
    uint32_t* voff;    // first word of layer l's values in d_values
    uint32_t* woff;    // first node of layer l's witness in d_witness (woff[l - 1] is its end; woff[0] = the count)
    uint32_t* node;    // [l][i]: position of the i-th distinct node of layer l
    uint32_t* nodek;   // [l][i]: entry of the block list its block is (layers >= b)
    uint32_t* wnode;   // position of a witness node
    uint32_t* wk;      // its block list entry | layer << 16
    uint32_t maxb, nq, wcap, top, b;
};
struct DcCols {
    uint16_t n[DC_LAYERS];  // columns of the tree at layer l
};

// Rank of a flag among the workgroup's 128 lanes (two waves) and the flags' masks: the level bitmask and popcount of
// k_plan_par, one ballot per wave.
__device__ __forceinline__ uint32_t dc_rank(bool f, uint64_t* m, uint64_t& m0, uint64_t& m1) {
    __syncthreads();  // the readers of the masks before
    const uint64_t bal = __ballot(f);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) m[w] = bal;
    __syncthreads();
    m0 = m[0];
    m1 = m[1];
    const uint64_t below = (w ? m1 : m0) & (((uint64_t)1 << lane) - 1);
    return (w ? (uint32_t)__popcll(m0) : 0u) + (uint32_t)__popcll(below);
}

// One workgroup of 128 lanes per proof: sort and de-duplicate the queries, then one lane per distinct leaf walks the layers.
// full: every block is in the list (the cap is being built); otherwise the blocks the queries touch.
__global__ __launch_bounds__(128) void k_dc_plan(const uint32_t* __restrict__ queries, const uint8_t* __restrict__ mask, DcCols nc, DcPlan pl,
                                                 uint32_t full, uint32_t* __restrict__ n_values, uint32_t nv_stride,
                                                 uint32_t* __restrict__ n_witness, uint32_t nw_stride) {
    __shared__ uint32_t q[128], s[128];
    __shared__ uint64_t m[2];
    const uint32_t p = blockIdx.x, tid = threadIdx.x;
    const uint32_t top = pl.top, b = pl.b, nq = pl.nq;
    uint32_t* nl = pl.nl + (size_t)p * DC_LAYERS;
    uint32_t* voff = pl.voff + (size_t)p * DC_LAYERS;
    uint32_t* woff = pl.woff + (size_t)p * DC_LAYERS;
    if (mask && !mask[p]) {
        if (tid < DC_LAYERS) nl[tid] = voff[tid] = woff[tid] = 0;
        if (tid == 0) {
            pl.cnt[p] = 0;
            n_values[(size_t)p * nv_stride] = 0;
            n_witness[(size_t)p * nw_stride] = 0;
        }
        return;
    }
    const uint32_t v = tid < nq ? queries[(size_t)p * nq + tid] & (uint32_t)(((uint64_t)1 << top) - 1) : 0xffffffffu;
    q[tid] = v;
    __syncthreads();
    if (tid < nq) {
        uint32_t r = 0;
        for (uint32_t j = 0; j < nq; j++) r += (q[j] < v || (q[j] == v && j < tid)) ? 1u : 0u;
        s[r] = v;
    } else {
        s[tid] = 0xffffffffu;
    }
    __syncthreads();
    uint64_t m0, m1;
    const uint32_t sv = s[tid];
    const bool first = tid < nq && (tid == 0 || s[tid - 1] != sv);
    const uint32_t r0 = dc_rank(first, m, m0, m1);
    const uint32_t n0 = (uint32_t)(__popcll(m0) + __popcll(m1));
    q[tid] = 0xffffffffu;
    __syncthreads();
    if (first) q[r0] = sv;
    __syncthreads();
    const bool act = tid < n0;
    const uint32_t leaf = q[tid];  // the tid-th distinct query, ascending; q is read-only from here
    // the block list
    const bool fb = act && (tid == 0 || (q[tid - 1] >> (top - b)) != (leaf >> (top - b)));
    const uint32_t rb = dc_rank(fb, m, m0, m1);
    uint32_t* blocks = pl.blocks + (size_t)p * pl.maxb;
    uint32_t k;
    if (full) {
        k = leaf >> (top - b);
        for (uint32_t i = tid; i < (1u << b); i += 128) blocks[i] = i;
        if (tid == 0) pl.cnt[p] = 1u << b;
    } else {
        k = rb + (fb ? 1u : 0u) - 1u;
        if (fb) blocks[rb] = leaf >> (top - b);
        if (tid == 0) pl.cnt[p] = (uint32_t)(__popcll(m0) + __popcll(m1));
    }
    // the layers, from the leaves down
    uint32_t* node = pl.node + (size_t)p * (top + 1) * nq;
    uint32_t* nodek = pl.nodek + (size_t)p * (top + 1) * nq;
    uint32_t* wnode = pl.wnode + (size_t)p * pl.wcap;
    uint32_t* wk = pl.wk + (size_t)p * pl.wcap;
    uint32_t vbase = 0, wbase = 0;
    for (uint32_t l = top;; l--) {
        const uint32_t x = leaf >> (top - l);
        const bool f = act && (tid == 0 || (q[tid - 1] >> (top - l)) != x);
        const uint32_t r = dc_rank(f, m, m0, m1);
        const uint32_t cnt = (uint32_t)(__popcll(m0) + __popcll(m1));
        if (f) {
            node[(size_t)l * nq + r] = x;
            nodek[(size_t)l * nq + r] = k;
        }
        if (tid == 0) {
            nl[l] = cnt;
            voff[l] = vbase;
            woff[l] = wbase;
        }
        vbase += cnt * nc.n[l];
        if (l == 0) break;
        // the sibling of a distinct node is queried iff it is the neighbouring distinct node
        bool miss = false;
        if (f) {
            bool present;
            if (x & 1) {
                present = tid > 0 && (q[tid - 1] >> (top - l)) == x - 1;
            } else {
                const uint32_t lane = tid & 63, w = tid >> 6;
                const uint64_t above = lane == 63 ? 0 : (w ? m1 : m0) & (~(uint64_t)0 << (lane + 1));
                uint32_t j = 128;
                if (above) j = w * 64 + (uint32_t)__ffsll((unsigned long long)above) - 1;
                else if (w == 0 && m1) j = 64 + (uint32_t)__ffsll((unsigned long long)m1) - 1;
                present = j < 128 && (q[j] >> (top - l)) == x + 1;  // a set bit is a distinct leaf's lane
            }
            miss = !present;
        }
        const uint32_t rw = dc_rank(miss, m, m0, m1);
        if (miss) {
            wnode[wbase + rw] = x ^ 1;
            wk[wbase + rw] = k | l << 16;
        }
        wbase += (uint32_t)(__popcll(m0) + __popcll(m1));
    }
    for (uint32_t l = top + 1 + tid; l < DC_LAYERS; l += 128) nl[l] = voff[l] = woff[l] = 0;
    if (tid == 0) {
        n_values[(size_t)p * nv_stride] = vbase;
        n_witness[(size_t)p * nw_stride] = wbase;
    }
}

// ---------------------------------------------------------------- the block-list forms of the commitment's kernels
// k_cm_fft_layer<false>, k_cm_fft_lds<false> and k_cm_hash_layer restated for a pass whose block kb of a proof is entry
// k0 + kb of that proof's block list (the absolute block index, for the twiddles and the block root's place); a block
// past the proof's count does not exist and its lanes leave.  They are kernels of their own, not a template argument of the
// commitment's, so that the commitment's kernels stay the instructions they were (wrapping them changed their register
// allocation); the butterflies, the row addressing and the hashing are the shared helpers of k_commit.hpp / merkle.hpp.
struct CmList {
    const uint32_t* list;  // [proofs][stride]
    const uint32_t* cnt;   // [proofs]
    uint32_t stride, k0, cols;  // cols: columns per proof of the rows (row -> proof)
    uint64_t cap_stride;   // words between two proofs' caps: the block roots go to the cap's layer b
};
__device__ __forceinline__ bool cm_block(const CmList& L, uint64_t p, uint32_t kb, uint32_t& blk) {
    const uint32_t k = L.k0 + kb;
    if (k >= L.cnt[p]) return false;
    blk = L.list[p * L.stride + k];
    return true;
}

__global__ __launch_bounds__(256) void k_dc_fft_layer(CmRows r, CmSrc s, const uint32_t* __restrict__ tw, uint32_t m, CmList L) {
    const uint32_t hl = r.log - 1;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (r.rows << hl)) return;
    const uint64_t row = t >> hl;
    const uint32_t j = (uint32_t)(t & ((1u << hl) - 1));
    const uint32_t p = ((j >> m) << (m + 1)) | (j & ((1u << m) - 1)), q = p + (1u << m);
    uint32_t kb, blk;
    uint32_t* d = cm_row(r, row, kb);
    if (!cm_block(L, row / r.nb / L.cols, kb, blk)) return;
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
    cm_butterfly<false>(a, b, tw[cm_tw_off(r.N, m) + ((((uint64_t)blk << r.log) + p) >> (m + 1))]);
    d[p] = a;
    d[q] = b;
}

__global__ __launch_bounds__(256) void k_dc_fft_lds(CmRows r, CmSrc s, const uint32_t* __restrict__ tw, uint32_t c, CmList L) {
    __shared__ uint32_t v[1u << CM_LDS_LOG];
    const uint32_t C = 1u << c, per_row_log = r.log - c;
    const uint64_t row = (uint64_t)blockIdx.x >> per_row_log;
    const uint32_t ch = blockIdx.x & ((1u << per_row_log) - 1);
    uint32_t kb, blk;
    uint32_t* d = cm_row(r, row, kb) + (uint64_t)ch * C;
    if (!cm_block(L, row / r.nb / L.cols, kb, blk)) return;  // the whole workgroup
    if (s.base) {
        uint32_t sc;
        const uint32_t* src = cm_src(s, row / r.nb, sc) + (uint64_t)ch * C;
        for (uint32_t i = threadIdx.x; i < C; i += 256) v[i] = m_mul(src[i], sc);
    } else {
        for (uint32_t i = threadIdx.x; i < C; i += 256) v[i] = d[i];
    }
    __syncthreads();
    const uint64_t abs0 = ((uint64_t)blk << r.log) + (uint64_t)ch * C;
    for (uint32_t k = 0; k < c; k++) {
        const uint32_t m = c - 1 - k;
        const uint32_t* twm = tw + cm_tw_off(r.N, m);
        for (uint32_t j = threadIdx.x; j < C / 2; j += 256) {
            const uint32_t p = ((j >> m) << (m + 1)) | (j & ((1u << m) - 1)), q = p + (1u << m);
            uint32_t a = v[p], b = v[q];
            cm_butterfly<false>(a, b, twm[(abs0 + p) >> (m + 1)]);
            v[p] = a;
            v[q] = b;
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < C; i += 256) d[i] = v[i];
}

// a.out at lw == 0: the caps of the pass's proofs; a.blk0 is not used.
__global__ __launch_bounds__(256) void k_dc_hash_layer(CmHashArgs a, CmList L) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)a.P * a.nb << a.lw)) return;
    const uint32_t j = (uint32_t)(t & ((1u << a.lw) - 1));
    const uint64_t rest = t >> a.lw;
    const uint32_t p = (uint32_t)(rest / a.nb), kb = (uint32_t)(rest - (uint64_t)p * a.nb);
    uint32_t blk;
    if (!cm_block(L, p, kb, blk)) return;
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
    uint32_t* o = a.lw ? a.out + t * 8 : a.out + p * L.cap_stride + (((uint64_t)1 << a.b) + blk) * 8;
    store_hash(o, h);
}

// Layer l < b of the caps of P proofs from layer l + 1; entry 0 is zero.  A proof without blocks (masked) is left alone.
__global__ __launch_bounds__(256) void k_dc_cap_level(uint32_t* __restrict__ cap, uint64_t cap_stride, uint32_t l, uint32_t P,
                                                      const uint32_t* __restrict__ cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)P << l)) return;
    const uint32_t p = (uint32_t)(t >> l), j = (uint32_t)(t & ((1u << l) - 1));
    if (!cnt[p]) return;
    uint32_t* c = cap + p * cap_stride;
    const uint32_t* in = c + (((uint64_t)2 << l) + 2 * j) * 8;
    store_hash(c + (((uint64_t)1 << l) + j) * 8, hash_tree<1>(load_hash(in), load_hash(in + 8)));
    if (l == 0) store_hash(c, zero8());
}

// A level of the cap a commitment leaves (rsv_commit_tree_cap_dev): in [P][2^l][8] -> layer l of d_cap of proofs p0 ..,
// zero for a masked proof; l == 0 also writes entry 0.
__global__ __launch_bounds__(256) void k_cm_cap_level(const uint32_t* __restrict__ in, uint64_t in_stride, uint32_t* __restrict__ cap,
                                                      uint64_t cap_stride, uint32_t l, uint32_t P, const uint8_t* __restrict__ mask, uint32_t p0) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)P << l)) return;
    const uint32_t p = (uint32_t)(t >> l), j = (uint32_t)(t & ((1u << l) - 1));
    const bool keep = !mask || mask[p0 + p];
    const Hash8 h = keep ? load_hash(in + p * in_stride + (uint64_t)j * 8) : zero8();
    uint32_t* c = cap + (uint64_t)(p0 + p) * cap_stride;
    store_hash(c + (((uint64_t)1 << l) + j) * 8, h);
    if (l == 0) store_hash(c, zero8());
}

// Rows of `width` words at base + i * stride, i < n, to zero.
__global__ __launch_bounds__(256) void k_dc_zero(uint32_t* __restrict__ base, uint64_t stride, uint64_t width, uint64_t n) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * width) return;
    const uint64_t i = t / width;
    base[i * stride + (t - i * width)] = 0;
}

struct DcOut {
    uint32_t* values;   // of the pass's first proof
    uint32_t* witness;
    uint64_t vstride, wstride;  // words between two proofs
};

// After layer a.lw + a.b of a pass (list entries k0 .. k0 + a.nb - 1 of a.P proofs): the witness nodes of that layer from
// a.out (layers above b) and the values of its columns from the LDE rows, one lane per word.
__global__ __launch_bounds__(256) void k_dc_gather(CmHashArgs a, DcPlan pl, DcOut o, uint32_t k0) {
    const uint32_t per = 8 + a.n_cols, l = a.lw + a.b;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)a.P * pl.nq * per) return;
    const uint32_t w = (uint32_t)(t % per);
    const uint64_t rest = t / per;
    const uint32_t i = (uint32_t)(rest % pl.nq), p = (uint32_t)(rest / pl.nq);
    if (w < 8) {
        if (!a.lw) return;  // layer b: from the cap
        const uint32_t* woff = pl.woff + (size_t)p * DC_LAYERS;
        const uint32_t slot = woff[l] + i;
        if (slot >= woff[l - 1]) return;
        const uint32_t kb = (pl.wk[(size_t)p * pl.wcap + slot] & 0xffffu) - k0;
        if (kb >= a.nb) return;  // another pass (wraps below k0)
        const uint32_t j = pl.wnode[(size_t)p * pl.wcap + slot] & ((1u << a.lw) - 1);
        o.witness[p * o.wstride + (uint64_t)slot * 8 + w] = a.out[((((uint64_t)p * a.nb + kb) << a.lw) + j) * 8 + w];
        return;
    }
    if (i >= pl.nl[(size_t)p * DC_LAYERS + l]) return;
    const size_t at = ((size_t)p * (pl.top + 1) + l) * pl.nq + i;
    const uint32_t kb = pl.nodek[at] - k0;
    if (kb >= a.nb) return;
    const uint32_t j = pl.node[at] & ((1u << a.lw) - 1);
    uint32_t c = w - 8, gi = 0;
    while (c >= a.g[gi].n_cols) c -= a.g[gi++].n_cols;
    const CmLayerCols& g = a.g[gi];
    o.values[p * o.vstride + pl.voff[(size_t)p * DC_LAYERS + l] + (uint64_t)i * a.n_cols + (w - 8)] =
        g.base[((uint64_t)p * g.n_cols + c) * g.pc_stride + ((uint64_t)kb << a.lw) + j];
}

// The witness nodes of layers <= b from the caps of P proofs, one lane per word.
__global__ __launch_bounds__(256) void k_dc_gather_cap(const uint32_t* __restrict__ cap, uint64_t cap_stride, DcPlan pl, DcOut o, uint32_t P) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t per = pl.nq * pl.b;  // at most nq nodes a layer
    if (t >= (uint64_t)P * per * 8) return;
    const uint32_t w = (uint32_t)(t & 7);
    const uint32_t i = (uint32_t)((t >> 3) % per), p = (uint32_t)((t >> 3) / per);
    const uint32_t* woff = pl.woff + (size_t)p * DC_LAYERS;
    const uint32_t slot = woff[pl.b] + i;
    if (slot >= woff[0]) return;
    const uint32_t l = pl.wk[(size_t)p * pl.wcap + slot] >> 16;
    const uint32_t x = pl.wnode[(size_t)p * pl.wcap + slot];
    o.witness[p * o.wstride + (uint64_t)slot * 8 + w] = cap[p * cap_stride + (((uint64_t)1 << l) + x) * 8 + w];
}

}  // namespace rsv
