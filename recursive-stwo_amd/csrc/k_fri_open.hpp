// k_fri_open.hpp — the opening of the FRI layer trees (fri_open_api.inc drives the launches; include/rsv.h:
// rsv_fri_open_dev): the plan of a (proof, tree)'s queries, the gather of the planned witness nodes after each rebuilt
// level, the gather of the planned values; and for rsv_fri_open_cap_dev the list of the subtrees that hold a planned node,
// their rebuilding in LDS and the gather from the caps (at the end of the file).
//
// stwo's pair-tree decommitment (consumed by SinglePairMerkleProof::from_stwo_proof).  A tree has leaves at layer `top`
// and a QM31 value per node at its data layers D: tree 0 (the first layer) top = M and D = the quotient columns' sizes,
// tree t >= 1 (inner layer t - 1) top = M - t and D = {top}.  With Q_l the distinct (query >> (top - l)) ascending and
// S_l = Q_l and their siblings at a data layer, Q_l elsewhere:
//   fri_witness    for l in D descending, the value at every x in S_l ascending that is not in Q_l;
//   hash_witness   for l = top - 1 .. 0 and x in S_l ascending, the nodes 2x, 2x + 1 that are not in S_(l+1).
// The queries sorted, a run of lanes with the same (leaf >> (top - l)) is a node of Q_l, and S_l of a data layer is the two
// children of every node of Q_(l-1).  So the plan gives the first lane of each run the run's work: at a data layer the
// run of the parent names the pair, at any other layer the run of the node itself; a lane names at most three witness
// nodes of a level (a queried child's missing grandchild, and both children of a sibling nobody queries).
#pragma once
#include "k_decommit.hpp"
#include "k_fri.hpp"

namespace rsv {

// The plan of every (proof, tree) (workspace), tree-minor: row pt = p * T + t.
struct FoPlan {
    uint32_t* woff;    // [pt][DC_LAYERS]: first node of layer l's witness in d_hash_witness (woff[l - 1] is its end; woff[0] = the count)
    uint32_t* wnode;   // [pt][wcap]: position of a witness node in its layer
    uint32_t* vnode;   // [pt][vcap]: position of a witness value in its layer
    uint32_t* vlayer;  // [pt][vcap]: that layer
    uint32_t T, M, nq, wcap, vcap, dmask;  // dmask bit l: tree 0 carries a value at layer l
};

// The masks of a flag over the workgroup's 128 lanes, one ballot per wave.
__device__ __forceinline__ void fo_masks(bool f, uint64_t* m, uint64_t& m0, uint64_t& m1) {
    __syncthreads();  // the readers of the masks before
    const uint64_t bal = __ballot(f);
    if ((threadIdx.x & 63) == 0) m[threadIdx.x >> 6] = bal;
    __syncthreads();
    m0 = m[0];
    m1 = m[1];
}
// The lane of the first set bit above this lane; 128 if there is none.
__device__ __forceinline__ uint32_t fo_next(uint64_t m0, uint64_t m1) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t above = lane == 63 ? 0 : (w ? m1 : m0) & (~(uint64_t)0 << (lane + 1));
    if (above) return w * 64 + (uint32_t)__ffsll((unsigned long long)above) - 1;
    if (w == 0 && m1) return 64 + (uint32_t)__ffsll((unsigned long long)m1) - 1;
    return 128;
}
// Counts of 0 .. 3 over the 128 lanes -> the sum of the lanes below and (total) of all: four ballots, the counts' two
// bits in each of the two waves.
__device__ __forceinline__ uint32_t fo_rank3(uint32_t cnt, uint64_t* m, uint32_t& total) {
    __syncthreads();
    const uint64_t lo = __ballot(cnt & 1u), hi = __ballot(cnt & 2u);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        m[2 * w] = lo;
        m[2 * w + 1] = hi;
    }
    __syncthreads();
    const uint32_t wave0 = (uint32_t)__popcll(m[0]) + 2u * (uint32_t)__popcll(m[1]);
    total = wave0 + (uint32_t)__popcll(m[2]) + 2u * (uint32_t)__popcll(m[3]);
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    return (w ? wave0 : 0u) + (uint32_t)__popcll(m[2 * w] & below) + 2u * (uint32_t)__popcll(m[2 * w + 1] & below);
}

// One workgroup of 128 lanes per (proof, tree): sort and de-duplicate the queries, then the first lane of every run names
// the run's witness values and witness nodes, layer by layer.  n_fri, n_hash [n][T].
__global__ __launch_bounds__(128) void k_fo_plan(const uint32_t* __restrict__ queries, const uint8_t* __restrict__ mask, FoPlan pl,
                                                 uint32_t* __restrict__ n_fri, uint32_t* __restrict__ n_hash) {
    __shared__ uint32_t q[128], s[128];
    __shared__ uint64_t m[4];
    const uint32_t p = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const size_t pt = (size_t)p * pl.T + t;
    const uint32_t top = pl.M - t, nq = pl.nq;
    const uint32_t data = t ? 1u << top : pl.dmask;
    uint32_t* woff = pl.woff + pt * DC_LAYERS;
    if (mask && !mask[p]) {
        if (tid < DC_LAYERS) woff[tid] = 0;
        if (tid == 0) n_fri[pt] = n_hash[pt] = 0;
        return;
    }
    const uint32_t v = tid < nq ? (queries[(size_t)p * nq + tid] & (uint32_t)(((uint64_t)1 << pl.M) - 1)) >> t : 0xffffffffu;
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
    const bool distinct = tid < nq && (tid == 0 || s[tid - 1] != sv);
    fo_masks(distinct, m, m0, m1);
    const uint32_t n0 = (uint32_t)(__popcll(m0) + __popcll(m1));
    const uint32_t r0 = (tid >> 6 ? (uint32_t)__popcll(m0) : 0u) + (uint32_t)__popcll((tid >> 6 ? m1 : m0) & (((uint64_t)1 << (tid & 63)) - 1));
    q[tid] = 0xffffffffu;
    __syncthreads();
    if (distinct) q[r0] = sv;
    __syncthreads();
    const bool act = tid < n0;
    const uint32_t leaf = q[tid];  // the tid-th distinct query, ascending; q is read-only from here
    // the node of layer l above the leaf of lane j < n0; whether this lane is the first of its run at layer l; the end of
    // a run among the runs whose first lanes are (m0, m1)
    const auto at = [&](uint32_t j, uint32_t l) { return q[j] >> (top - l); };
    const auto first_at = [&](uint32_t l) { return act && (tid == 0 || at(tid - 1, l) != at(tid, l)); };
    const auto end_of = [&](uint64_t a0, uint64_t a1) { return min(fo_next(a0, a1), n0); };

    // fri_witness: at a data layer l, of the pair under every node y of Q_(l-1) the child no query reaches
    uint32_t* vnode = pl.vnode + pt * pl.vcap;
    uint32_t* vlayer = pl.vlayer + pt * pl.vcap;
    uint32_t vbase = 0;
    for (uint32_t l = top; l >= 1; l--) {
        if (!(data >> l & 1u)) continue;
        const bool f = first_at(l - 1);
        fo_masks(f, m, m0, m1);
        uint32_t cnt = 0, x = 0;
        if (f) {
            const uint32_t e = end_of(m0, m1), y = leaf >> (top - l + 1);
            if (at(tid, l) != 2 * y) {
                cnt = 1;
                x = 2 * y;
            } else if (at(e - 1, l) != 2 * y + 1) {
                cnt = 1;
                x = 2 * y + 1;
            }
        }
        uint32_t total;
        const uint32_t r = fo_rank3(cnt, m, total);
        if (cnt && vbase + r < pl.vcap) {
            vnode[vbase + r] = x;
            vlayer[vbase + r] = l;
        }
        vbase += total;
    }

    // hash_witness: the nodes of layer c = l + 1 that the nodes of S_l need and S_c does not hold
    uint32_t* wnode = pl.wnode + pt * pl.wcap;
    uint32_t wbase = 0;
    for (uint32_t c = top; c >= 1; c--) {
        const uint32_t l = c - 1;
        if (tid == 0) woff[c] = wbase;
        const bool pair_below = data >> c & 1u;  // S_c holds both children of a queried node
        // of the left and of the right node of a pair (of the one node elsewhere): how many witness nodes, and the first —
        // a second one is its right neighbour
        uint32_t na = 0, a0 = 0, nb = 0, b0 = 0;
        if (l >= 1 && (data >> l & 1u)) {
            // S_l: the pair 2y, 2y + 1 under every node y of Q_(l-1).  The run of y is [tid, e), of 2y [tid, mid), of
            // 2y + 1 [mid, e); a child without a run is a sibling nobody queries: both its children are witnesses.
            const bool f = first_at(l - 1);
            uint64_t c0, c1;
            fo_masks(f, m, m0, m1);
            fo_masks(first_at(l), m, c0, c1);
            if (f) {
                const uint32_t e = end_of(m0, m1), y = leaf >> (top - l + 1);
                const bool has_l = at(tid, l) == 2 * y, has_r = at(e - 1, l) == 2 * y + 1;
                const uint32_t mid = has_l ? (has_r ? end_of(c0, c1) : e) : tid;
                if (!has_l) {
                    na = 2;
                    a0 = 4 * y;
                } else if (!pair_below && at(tid, c) == at(mid - 1, c)) {
                    na = 1;
                    a0 = at(tid, c) ^ 1u;
                }
                if (!has_r) {
                    nb = 2;
                    b0 = 4 * y + 2;
                } else if (!pair_below && at(mid, c) == at(e - 1, c)) {
                    nb = 1;
                    b0 = at(mid, c) ^ 1u;
                }
            }
        } else {
            // S_l = Q_l: of a node's children the one no query reaches
            const bool f = first_at(l);
            fo_masks(f, m, m0, m1);
            if (f && !pair_below) {
                const uint32_t e = end_of(m0, m1);
                if (at(tid, c) == at(e - 1, c)) {
                    na = 1;
                    a0 = at(tid, c) ^ 1u;
                }
            }
        }
        uint32_t total;
        const uint32_t r = wbase + fo_rank3(na + nb, m, total);
        for (uint32_t k = 0; k < na; k++)
            if (r + k < pl.wcap) wnode[r + k] = a0 + k;
        for (uint32_t k = 0; k < nb; k++)
            if (r + na + k < pl.wcap) wnode[r + na + k] = b0 + k;
        wbase += total;
    }
    for (uint32_t l = top + 1 + tid; l < DC_LAYERS; l += 128) woff[l] = 0;
    if (tid == 0) {
        woff[0] = wbase;
        n_fri[pt] = vbase;
        n_hash[pt] = wbase;
    }
}

// After layers l (hi [P][2^l][8]) and l - 1 (lo [P][2^(l-1)][8]; nullptr: layer l alone) of tree t of a pass of P proofs,
// k_fr_hash_layer's: the planned witness nodes of those layers to their slots, one lane per word; at most 3 nq nodes a
// layer.  pl and out (d_hash_witness) from the pass's first proof.
__global__ __launch_bounds__(256) void k_fo_gather(const uint32_t* __restrict__ hi, const uint32_t* __restrict__ lo, uint32_t l, uint32_t t,
                                                   uint32_t P_, FoPlan pl, uint32_t* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t per = 6 * pl.nq;
    if (g >= (uint64_t)P_ * per * 8) return;
    const uint32_t w = (uint32_t)(g & 7);
    const uint32_t i = (uint32_t)((g >> 3) % per), p = (uint32_t)((g >> 3) / per);
    const size_t pt = (size_t)p * pl.T + t;
    const uint32_t* woff = pl.woff + pt * DC_LAYERS;
    const uint32_t slot = woff[l] + i, mid = woff[l - 1];
    if (slot >= (lo ? woff[l - 2] : mid) || slot >= pl.wcap) return;
    const uint32_t x = pl.wnode[pt * pl.wcap + slot];
    const uint32_t* src = slot < mid ? hi + ((((uint64_t)p) << l) + x) * 8 : lo + ((((uint64_t)p) << (l - 1)) + x) * 8;
    out[(pt * pl.wcap + slot) * 8 + w] = src[w];
}

// Where the values live: the quotient columns (col_at[l]: the column of layer l) and the inner layers, as
// rsv_fri_commit_dev takes and leaves them.
struct FoData {
    const uint32_t *quot, *layers;
    uint64_t qstride, lstride;
    uint64_t col_at[DC_LAYERS];
};

// d_fri_witness [n][T][vcap][4], one lane per word: the planned value's coordinate, zero past the count.
__global__ __launch_bounds__(256) void k_fo_values(FoData d, FoPlan pl, const uint32_t* __restrict__ n_fri, uint32_t n, uint32_t* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (uint64_t)n * pl.T * pl.vcap * 4) return;
    const uint32_t j = (uint32_t)(g & 3);
    const uint32_t slot = (uint32_t)((g >> 2) % pl.vcap);
    const uint64_t pt = (g >> 2) / pl.vcap;
    const uint64_t p = pt / pl.T;
    const uint32_t t = (uint32_t)(pt - p * pl.T);
    uint32_t v = 0;
    if (slot < n_fri[pt]) {
        const uint32_t l = pl.vlayer[pt * pl.vcap + slot], x = pl.vnode[pt * pl.vcap + slot];
        const uint32_t* s = t ? d.layers + p * d.lstride + fr_layer_off(pl.M, l) : d.quot + p * d.qstride + d.col_at[l];
        v = s[((uint64_t)j << l) + x];
    }
    out[g] = v;
}

// ---------------------------------------------------------------- the cap form (rsv_fri_open_cap_dev)
// rsv_fri_commit_cap_dev keeps layers 1 .. c of every tree, c = max(top - h, 0), in d_caps; below layer c a tree is 2^c
// subtrees of 2^(top - c) leaves.  A planned node above layer c comes from the rebuilt subtree under its layer-c ancestor
// (k_fo_sublist names those, k_fo_subtree hashes them in LDS), a planned node at a layer <= c from the cap (k_fo_cap_gather).
// FoCaps, fo_cap_layers and fo_cap_at, the layout of d_caps, are k_fri.hpp's: the commitment's kernels write it.
constexpr uint32_t FO_MAX_SUB_LOG = 8;  // RSV_MAX_FRI_SUB_LOG

// The subtrees of every (proof, tree) (workspace): at most 2 nq, S_c holding every one of them.
struct FoSubs {
    uint32_t* cnt;  // [pt]
    uint32_t* ids;  // [pt][2 nq] ascending: positions in layer c
};

// One workgroup of 128 lanes per (proof, tree): the distinct layer-c ancestors of the planned nodes above layer c (the
// slots below woff[c]).  A layer's nodes are ascending, so is what lies above them in layer c: a slot opens a subtree when
// its neighbour to the left lies under another one and a search of every layer before it finds none under the same.
__global__ __launch_bounds__(128) void k_fo_sublist(FoPlan pl, uint32_t h, FoSubs sb) {
    __shared__ uint32_t ids[2 * 128];
    __shared__ uint32_t cnt;
    const uint32_t p = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const size_t pt = (size_t)p * pl.T + t;
    const uint32_t top = pl.M - t, c = fo_cap_layers(top, h), cap = 2 * pl.nq;
    const uint32_t* woff = pl.woff + pt * DC_LAYERS;
    const uint32_t* wnode = pl.wnode + pt * pl.wcap;
    const uint32_t end = min(woff[c], pl.wcap);
    if (tid == 0) cnt = 0;
    __syncthreads();
    for (uint32_t s = tid; s < end; s += 128) {
        uint32_t l = top;  // layer l's nodes are the slots woff[l] .. woff[l - 1] - 1
        while (l > c + 1 && s >= woff[l - 1]) l--;
        const uint32_t a = wnode[s] >> (l - c);
        bool opens = s == woff[l] || (wnode[s - 1] >> (l - c)) != a;
        for (uint32_t u = top; opens && u > l; u--) {
            const uint32_t stop = min(woff[u - 1], end);
            uint32_t lo = woff[u], hi = stop;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((wnode[mid] >> (u - c)) < a) lo = mid + 1;
                else hi = mid;
            }
            opens = !(lo < stop && (wnode[lo] >> (u - c)) == a);
        }
        if (opens) {
            const uint32_t k = atomicAdd(&cnt, 1u);
            if (k < cap) ids[k] = a;
        }
    }
    __syncthreads();
    const uint32_t m = min(cnt, cap);
    for (uint32_t i = tid; i < m; i += 128) {
        const uint32_t v = ids[i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < m; j++) r += ids[j] < v ? 1u : 0u;
        sb.ids[pt * cap + r] = v;
    }
    if (tid == 0) sb.cnt[pt] = m;
}

// One workgroup of 256 lanes per (proof, tree, listed subtree): fr_node (k_fri.hpp) of the levels top .. c + 1 of the subtree
// under node `id` of layer c, a lane per node, every level kept in LDS (word-major, level c + e at entries 2^e + j; the subtree's
// own root is a node of the cap, or the tree's root, and is not hashed); then the planned nodes that lie in this subtree
// to their slots of d_hash_witness, a lane per word.  out: d_hash_witness of proof 0.
__global__ __launch_bounds__(256) void k_fo_subtree(FoData d, FoPlan pl, uint32_t h, FoSubs sb, uint32_t* __restrict__ out) {
    __shared__ uint32_t node[8][2u << FO_MAX_SUB_LOG];
    const uint32_t cap = 2 * pl.nq, tid = threadIdx.x;
    const uint64_t pt = blockIdx.x / cap;
    const uint32_t k = blockIdx.x - (uint32_t)pt * cap;
    if (k >= sb.cnt[pt]) return;  // the whole workgroup
    const uint64_t p = pt / pl.T;
    const uint32_t t = (uint32_t)(pt - p * pl.T);
    const uint32_t top = pl.M - t, c = fo_cap_layers(top, h), sl = top - c;
    const uint32_t id = sb.ids[pt * cap + k];
    if (id >> c) return;  // not a node of layer c: nothing is read past a column's end
    for (uint32_t e = sl; e >= 1; e--) {
        const uint32_t l = c + e;
        if (tid < (1u << e)) {
            const Hash8 v = fr_node(
                e == sl,
                [&](uint32_t* x) {
                    if (!(t == 0 ? pl.dmask >> l & 1u : l == top)) return false;
                    const uint32_t* s = (t ? d.layers + p * d.lstride + fr_layer_off(pl.M, l) : d.quot + p * d.qstride + d.col_at[l]) + (((uint64_t)id << e) + tid);
#pragma unroll
                    for (int j = 0; j < 4; j++) x[j] = s[(uint64_t)j << l];
                    return true;
                },
                [&](Hash8& a, Hash8& b) {
                    const uint32_t at = (2u << e) + 2 * tid;
#pragma unroll
                    for (int w = 0; w < 8; w++) {
                        a.w[w] = node[w][at];
                        b.w[w] = node[w][at + 1];
                    }
                });
#pragma unroll
            for (int w = 0; w < 8; w++) node[w][(1u << e) + tid] = v.w[w];
        }
        __syncthreads();
    }
    const uint32_t* woff = pl.woff + pt * DC_LAYERS;
    const uint32_t* wnode = pl.wnode + pt * pl.wcap;
    const uint32_t end = min(woff[c], pl.wcap);
    for (uint32_t g = tid; g < end * 8; g += 256) {
        const uint32_t slot = g >> 3, w = g & 7;
        uint32_t l = top;
        while (l > c + 1 && slot >= woff[l - 1]) l--;
        const uint32_t e = l - c, x = wnode[slot];
        if ((x >> e) == id) out[(pt * pl.wcap + slot) * 8 + w] = node[w][(1u << e) + (x & ((1u << e) - 1))];
    }
}

// The planned nodes of the layers <= c from the caps, one lane per word of d_hash_witness [n][T][wcap][8].
__global__ __launch_bounds__(256) void k_fo_cap_gather(FoCaps kc, FoPlan pl, uint32_t n, uint32_t* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (uint64_t)n * pl.T * pl.wcap * 8) return;
    const uint32_t w = (uint32_t)(g & 7);
    const uint32_t slot = (uint32_t)((g >> 3) % pl.wcap);
    const uint64_t pt = (g >> 3) / pl.wcap;
    const uint64_t p = pt / pl.T;
    const uint32_t t = (uint32_t)(pt - p * pl.T);
    const uint32_t c = fo_cap_layers(pl.M - t, kc.h);
    const uint32_t* woff = pl.woff + pt * DC_LAYERS;
    if (c == 0 || slot < woff[c] || slot >= woff[0]) return;
    uint32_t l = c;
    while (l > 1 && slot >= woff[l - 1]) l--;
    const uint32_t x = pl.wnode[pt * pl.wcap + slot];
    out[g] = kc.caps[fo_cap_at(kc, t, l, p) + (uint64_t)x * 8 + w];
}

}  // namespace rsv
