// k_fri.hpp — the commit phase of FRI of the next proof: the DEEP quotient columns over their whole domains, the first
// layer's and the inner layers' Merkle trees, the transcript between them, the two folds and the last layer's polynomial
// (fri_api.inc drives the launches; include/rsv.h: rsv_fri_quotients_dev, rsv_fri_commit_dev, rsv_witness_fri_dev).
//
// The definition is the verifier's (k_query.hpp: the quotient constants, the row quotient and the folds per query),
// evaluated at every position instead of the queried ones.
//
// Quotients.  One QM31 column per distinct LDE log size N.  Sample k of a column (value v at the point (px, py), both
// QM31 = (CM31, CM31)) has the line coefficients a = w v.b, b = w (v.a py.b - v.b py.a), c = w py.b with w the running
// power of `after`, starting at -2u for every column and advancing through the batches (one per point) in order.  At
// position q, whose domain point is the M31 point (x, y),
//   value = sum over batches of (sum_k c_k row[col_k] - (y sum_k a_k + sum_k b_k)) / den,
//   den   = (px.a - x) py.b - (py.a - y) px.b = D0 - x py.b + y px.b          (CM31),
// so a batch is a dot product of M31 row words with wave-uniform QM31 coefficients (four multiply-accumulates per
// column into unreduced u64 sums, as k_sp_dot's), one affine term and one CM31 inverse.  k_fr_consts forms c_k, sum a,
// sum b, D0 once per proof; the row words are the commitment's LDE, streamed in blocks (k_commit.hpp), never whole.
// The domain point comes from the forward twiddle table of the domain 2^N the FFT uses anyway: y of position q is layer
// 0's entry q >> 1, negated for odd q; x is layer 1's entry q >> 2, negated where bit 1 of q is set.
//
// Folds (bit-reversed storage, pair (2k, 2k + 1)).  Circle to line, column of log size l: (f0 + f1) + alpha (f0 - f1) / y,
// 1 / y = entry k of layer 0 of the inverse table of 2^l.  Line, layer of log size l: (f0 + f1) + alpha (f0 - f1) / x,
// 1 / x = entry k of layer 1 of the inverse table of 2^(l + 1).  No factor 1/2.
//
// Three forms of the commit phase (per layer; the same keeping the caps; the tail form) and the opening (k_fri_open.hpp) must
// agree bit for bit, so every step has one __device__ definition here and a per-layer kernel that is index arithmetic around
// it: fr_node (k_fr_hash_layer; fr_lds_tree, k_fo_subtree), fr_draw_one (k_fr_draw), fr_fold_pair and fr_fold_join
// (k_fr_fold), fr_line_pair (k_fr_line_layer), fr_last_word (k_fr_last), fr_mix_last (k_fr_mix_last); k_fr_tree_top and
// k_fr_tail are loops around the same calls.
#pragma once
#include "k_commit.hpp"
#include "k_sample.hpp"

namespace rsv {

constexpr uint32_t FR_MAX_GROUPS = 12;  // RSV_MAX_COMMIT_GROUPS for a caller; the chain has eleven (fri_api.inc)
constexpr uint32_t FR_MAX_POINTS = 4;   // RSV_MAX_SAMPLE_POINTS
constexpr uint32_t FR_HDR_WORDS = 16;   // per batch: sum a [4], sum b [4], D0 [2], py.b [2], px.b [2], 2 unused
constexpr uint32_t FR_TERMS_AT = FR_MAX_POINTS * FR_HDR_WORDS;  // the terms' c follow the four headers, four words each

// One column group of a quotient column.  Point k applies to its columns lo[k] .. hi[k] - 1 (hi <= lo: to none); the
// sampled value of column c at point k is entry entry[k] + (c - lo[k]) * step[k] (four words each) of proof p's values at
// samples + p * sstride.  ext: the extended rows of the pass, proof p (of the pass), column c, row r of the block at
// ext + p * pstride + (c << rlog) + r (pstride 0: shared by every proof).
struct FrGroup {
    const uint32_t* ext;
    uint64_t pstride;
    const uint32_t* samples;
    uint64_t sstride;
    uint32_t n_cols;
    uint32_t lo[FR_MAX_POINTS], hi[FR_MAX_POINTS], entry[FR_MAX_POINTS], step[FR_MAX_POINTS];
};
struct FrCol {
    FrGroup g[FR_MAX_GROUPS];
    uint32_t ng, np;        // groups of this size, points
    uint32_t par_words;     // FR_TERMS_AT + 4 * terms
    uint32_t p0;            // the pass's first proof (mask, points, after, samples are indexed p0 + p)
    const uint8_t* mask;
    uint32_t* par;          // [proofs of the pass][par_words]
};

// One lane per proof of the pass: points [n][np][8] (x then y), after [n][4]; any u32 is taken mod P.
__global__ __launch_bounds__(64) void k_fr_consts(FrCol a, const uint32_t* __restrict__ points, const uint32_t* __restrict__ after,
                                                  uint32_t n_pass) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pass || (a.mask && !a.mask[a.p0 + p])) return;
    const uint64_t pp = a.p0 + p;
    uint32_t* par = a.par + (uint64_t)p * a.par_words;
    const QM31 step = sp_load_q(after + pp * 4);
    QM31 w = q_mk(0, 0, P - 2, 0);
    uint32_t t = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < a.np; k++) {
        const uint32_t* pt = points + (pp * a.np + k) * 8;
        const QM31 px = sp_load_q(pt), py = sp_load_q(pt + 4);
        QM31 sa = q_zero(), sb = q_zero();
#pragma unroll 1
        for (uint32_t gi = 0; gi < a.ng; gi++) {
            const FrGroup& g = a.g[gi];
            const uint32_t* sv = g.samples + pp * g.sstride;
#pragma unroll 1
            for (uint32_t c = g.lo[k]; c < g.hi[k]; c++, t++) {
                const QM31 v = sp_load_q(sv + ((uint64_t)g.entry[k] + (uint64_t)(c - g.lo[k]) * g.step[k]) * 4);
                sa = q_add(sa, q_mul_c(w, v.b));
                sb = q_add(sb, q_mul_c(w, c_sub(c_mul(v.a, py.b), c_mul(v.b, py.a))));
                const QM31 cc = q_mul_c(w, py.b);
                uint32_t* o = par + FR_TERMS_AT + t * 4;
                o[0] = cc.a.a; o[1] = cc.a.b; o[2] = cc.b.a; o[3] = cc.b.b;
                w = q_mul(w, step);
            }
        }
        const CM31 d0 = c_sub(c_mul(px.a, py.b), c_mul(py.a, px.b));
        uint32_t* h = par + k * FR_HDR_WORDS;
        h[0] = sa.a.a; h[1] = sa.a.b; h[2] = sa.b.a; h[3] = sa.b.b;
        h[4] = sb.a.a; h[5] = sb.a.b; h[6] = sb.b.a; h[7] = sb.b.b;
        h[8] = d0.a; h[9] = d0.b; h[10] = py.b.a; h[11] = py.b.b; h[12] = px.b.a; h[13] = px.b.b; h[14] = 0u; h[15] = 0u;
    }
}

// The rows of one pass of one quotient column: 2^rlog rows per proof from position row0 of the domain 2^N.
struct FrRows {
    FrCol col;
    uint32_t rlog, N;
    uint64_t row0;
    const uint32_t* tw;  // forward twiddle table of the domain 2^N
    uint32_t* quot;      // the column of proof p0: coordinate j of proof p0 + p at quot + p * qstride + (j << N)
    uint64_t qstride;
};

// One lane per (proof, row): the quotient column's value at the row's position; zeros for a masked proof.  The sums are
// CoAcc's: a folded remainder < 2^34 plus at most four products of canonical words (the LDE's m_* results, k_fr_consts'
// q_mul results).
__global__ __launch_bounds__(256) void k_fr_rows(FrRows a) {
    const uint32_t bpp = a.rlog > 8 ? 1u << (a.rlog - 8) : 1u;  // workgroups per proof: a wave's rows belong to one proof
    const uint32_t p = blockIdx.x / bpp, r = (blockIdx.x - p * bpp) * 256 + threadIdx.x;
    if (r >= (1u << a.rlog)) return;
    const uint64_t pos = a.row0 + r;
    uint32_t* o = a.quot + (uint64_t)p * a.qstride + pos;
    QM31 v = q_zero();
    if (!(a.col.mask && !a.col.mask[a.col.p0 + p])) {
        const uint32_t* par = a.col.par + (uint64_t)p * a.col.par_words;
        uint32_t y = a.tw[cm_tw_off(a.N, 0) + (pos >> 1)], x = a.tw[cm_tw_off(a.N, 1) + (pos >> 2)];
        if (pos & 1) y = m_neg(y);
        if (pos & 2) x = m_neg(x);
        const uint32_t* ct = par + FR_TERMS_AT;
#pragma unroll 1
        for (uint32_t k = 0; k < a.col.np; k++) {
            uint64_t acc[4] = {0, 0, 0, 0};
            uint32_t nt = 0;
#pragma unroll 1
            for (uint32_t gi = 0; gi < a.col.ng; gi++) {
                const FrGroup& g = a.col.g[gi];
                const uint32_t* e = g.ext + p * g.pstride + r;
#pragma unroll 4
                for (uint32_t c = g.lo[k]; c < g.hi[k]; c++, nt++, ct += 4) {
                    const uint32_t w = e[(uint64_t)c << a.rlog];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        acc[j] += (uint64_t)w * ct[j];
                        if ((nt & 3) == 3) acc[j] = sp_fold(acc[j]);
                    }
                }
            }
            if (!nt) continue;
            const uint32_t* h = par + k * FR_HDR_WORDS;
            const QM31 sum = q_mk(sp_canon(sp_fold(acc[0])), sp_canon(sp_fold(acc[1])), sp_canon(sp_fold(acc[2])), sp_canon(sp_fold(acc[3])));
            const QM31 lin = q_add(q_mul_m(q_mk(h[0], h[1], h[2], h[3]), y), q_mk(h[4], h[5], h[6], h[7]));
            const CM31 den = c_add(c_sub(c_mk(h[8], h[9]), c_mul_m(c_mk(h[10], h[11]), x)), c_mul_m(c_mk(h[12], h[13]), y));
            v = q_add(v, q_mul_c(q_sub(sum, lin), c_inv(den)));
        }
    }
    o[0] = v.a.a;
    o[(uint64_t)1 << a.N] = v.a.b;
    o[(uint64_t)2 << a.N] = v.b.a;
    o[(uint64_t)3 << a.N] = v.b.b;
}

// ---------------------------------------------------------------- layer trees
// hash_node of one node of a layer tree, the one definition every form of the commit phase and the opening hash with.
// col(v): whether the node's level carries a column, and then the node's QM31 of it in v — four M31 columns to the hash, as
// k_cm_hash_layer takes a group of four.  kids(a, b): the node's children, asked for above the leaves only.  Callbacks, not
// values: each caller's loads stay inside the branch that needs them.
template <class Col, class Kids>
__device__ __forceinline__ Hash8 fr_node(bool leaf, Col col, Kids kids) {
    uint32_t v[4];
    const bool has = col(v);
    Hash8 d = zero8();
    if (has) d = sponge_capacity4<1>(v[0], v[1], v[2], v[3]);
    Hash8 h;
    if (leaf) {
        h = leaf_from_capacity<1>(d);
    } else {
        Hash8 a, b;
        kids(a, b);
        h = hash_tree<1>(a, b);
        if (has) h = combine_with_column<1>(h, d);
    }
    return h;
}

// fr_node of every node of one layer of P trees, one lane per node: out [P][2^l][8]; child [P][2^(l+1)][8], nullptr at
// the leaves; data (may be nullptr): the one QM31 column this layer carries, coordinate j of proof p, node i at
// data + p * dstride + (j << l) + i.
__global__ __launch_bounds__(256) void k_fr_hash_layer(const uint32_t* __restrict__ data, uint64_t dstride, uint32_t l, uint32_t P_,
                                                       const uint32_t* __restrict__ child, uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)P_ << l)) return;
    const Hash8 h = fr_node(
        !child,
        [&](uint32_t* v) {
            if (!data) return false;
            const uint64_t p = t >> l, i = t & (((uint64_t)1 << l) - 1);
            const uint32_t* s = data + p * dstride + i;
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = s[(uint64_t)j << l];
            return true;
        },
        [&](Hash8& a, Hash8& b) {
            a = load_hash(child + t * 16);
            b = load_hash(child + t * 16 + 8);
        });
    store_hash(out + t * 8, h);
}

// Where the channel steps of the layers read and write, for the proofs of a pass: chan [P][16] (merkle.hpp: channel_load), read
// and updated; a layer's root to roots + p * rstride, its alpha to alphas + p * astride.
struct FrDraw {
    const uint8_t* mask;
    uint32_t* chan;
    uint32_t* roots;  // of layer 0
    uint64_t rstride;
    uint32_t* alphas;
    uint64_t astride;
    uint8_t* low;  // the proofs' low-degree flags; layer 0's step sets them
    // the same, with layer idx where layer 0 was
    __host__ __device__ FrDraw layer(uint32_t idx) const { return {mask, chan, roots + idx * 8, rstride, alphas + idx * 4, astride, idx ? nullptr : low}; }
};
// The channel step of one layer (d: FrDraw::layer's) of proof p of the pass, by one lane: mix the layer's root (root(), asked
// for when the proof is kept), draw alpha -> alpha.  A masked proof: zeros in the channel, the root and alpha.  Layer 0 also
// sets the proof's low-degree flag to 1 (0 for a masked proof) before fr_last_word clears it.
template <class Root>
__device__ __forceinline__ QM31 fr_draw_one(const FrDraw& d, uint32_t p, bool keep, Root root) {
    uint32_t* co = d.chan + (size_t)p * 16;
    uint32_t* ro = d.roots + p * d.rstride;
    uint32_t* ao = d.alphas + p * d.astride;
    if (d.low) d.low[p] = keep ? 1 : 0;
    if (!keep) {
#pragma unroll
        for (int i = 0; i < 16; i++) co[i] = 0u;
        store_hash(ro, zero8());
#pragma unroll
        for (int i = 0; i < 4; i++) ao[i] = 0u;
        return q_zero();
    }
    Channel<0> ch = channel_load(co);
    const Hash8 r = root();
    ch.mix(r);
    const Hash8 dr = ch.draw();
    channel_store(co, ch);
    store_hash(ro, r);
#pragma unroll
    for (int i = 0; i < 4; i++) ao[i] = dr.w[i];
    return q_lo(dr);
}

// fr_draw_one of one layer, one lane per proof of the pass; root [P][8].
__global__ __launch_bounds__(64) void k_fr_draw(const uint32_t* __restrict__ root, const uint8_t* __restrict__ mask, uint32_t P_,
                                                uint32_t* __restrict__ chan, uint32_t* __restrict__ roots, uint64_t rstride,
                                                uint32_t* __restrict__ alphas, uint64_t astride, uint8_t* __restrict__ low) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P_) return;
    fr_draw_one(FrDraw{mask, chan, roots, rstride, alphas, astride, low}, p, !mask || mask[p], [&] { return load_hash(root + (size_t)p * 8); });
}

// Where inner layer M - 1 - l (log size l < M) begins in a proof's d_layers, the layers M - 1, M - 2, ... one after
// another, each [4][2^size]: 4 (2^M - 2^(l+1)) words.
__host__ __device__ inline uint64_t fr_layer_off(uint32_t M, uint32_t l) { return ((uint64_t)4 << M) - ((uint64_t)8 << l); }

// ---------------------------------------------------------------- the caps of the layer trees
// rsv_fri_commit_cap_dev keeps layers 1 .. c of every tree, c = max(top - h, 0), in d_caps (k_fri_open.hpp reads them).
constexpr uint32_t FO_MAX_TREES = 29;   // 1 + RSV_MAX_FRI_INNER

__host__ __device__ inline uint32_t fo_cap_layers(uint32_t top, uint32_t h) { return top > h ? top - h : 0; }

// d_caps, level-major and proof-minor: tree after tree, in a tree layer 1 .. c one after another, a layer [n][2^l][8] — what
// k_fr_hash_layer writes as `out` and reads as `child`.
struct FoCaps {
    const uint32_t* caps;
    uint64_t tree_at[FO_MAX_TREES];  // words before tree t
    uint64_t n;
    uint32_t h;
};
// Where proof p's nodes of layer l (1 <= l <= c) of tree t begin.
__host__ __device__ inline uint64_t fo_cap_at(const FoCaps& k, uint32_t t, uint32_t l, uint64_t p) {
    return k.tree_at[t] + k.n * (((uint64_t)8 << l) - 16) + ((p << l) << 3);
}

// ---------------------------------------------------------------- folds
// A set of P QM31 vectors of 2^l values: coordinate j of proof p, value i at base + p * stride + (j << l) + i.
struct FrVec {
    uint32_t* base;
    uint64_t stride;
};
__device__ __forceinline__ QM31 fr_ld(const uint32_t* s, uint32_t l) {
    return q_mk(s[0], s[(uint64_t)1 << l], s[(uint64_t)2 << l], s[(uint64_t)3 << l]);
}
__device__ __forceinline__ void fr_st(uint32_t* d, uint32_t l, QM31 v) {
    d[0] = v.a.a;
    d[(uint64_t)1 << l] = v.a.b;
    d[(uint64_t)2 << l] = v.b.a;
    d[(uint64_t)3 << l] = v.b.b;
}

// One pair of a fold: (f0 + f1) + alpha (f0 - f1) winv, winv = 1 / y of the pair (circle to line) or 1 / x (line).
__device__ __forceinline__ QM31 fr_fold_pair(QM31 f0, QM31 f1, uint32_t winv, QM31 alpha) {
    return q_add(q_add(f0, f1), q_mul(q_mul_m(q_sub(f0, f1), winv), alpha));
}
// A folded quotient column joining the running evaluation: alpha^2 run + col.
__device__ __forceinline__ QM31 fr_fold_join(QM31 run, QM31 col, QM31 alpha) { return q_add(q_mul(q_mul(alpha, alpha), run), col); }

// src (log size l) -> dst (log size l - 1), one lane per (proof, k): fr_fold_pair with winv[k], winv the layer of the inverse
// twiddle table that holds 1 / y or 1 / x.  JOIN: dst = fr_fold_join of dst and that.  alpha: alphas + p * astride.  A masked
// proof gets zeros.
template <bool JOIN>
__global__ __launch_bounds__(256) void k_fr_fold(FrVec src, FrVec dst, uint32_t l, uint32_t P_, const uint32_t* __restrict__ winv,
                                                 const uint32_t* __restrict__ alphas, uint64_t astride, const uint8_t* __restrict__ mask) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)P_ << (l - 1))) return;
    const uint64_t p = t >> (l - 1), k = t & (((uint64_t)1 << (l - 1)) - 1);
    uint32_t* d = dst.base + p * dst.stride + k;
    QM31 v = q_zero();
    if (!mask || mask[p]) {
        const uint32_t* s = src.base + p * src.stride + 2 * k;
        const QM31 f0 = fr_ld(s, l), f1 = fr_ld(s + 1, l);
        const uint32_t* ap = alphas + p * astride;
        const QM31 alpha = q_mk(ap[0], ap[1], ap[2], ap[3]);
        v = fr_fold_pair(f0, f1, winv[k], alpha);
        if (JOIN) v = fr_fold_join(fr_ld(d, l - 1), v, alpha);
    }
    fr_st(d, l - 1, v);
}

// ---------------------------------------------------------------- last layer
// Pair j of inverse butterfly layer m of the line interpolation of a vector v of 2^L words, in place.  The line domain of 2^L
// points is the x-projection of the circle domain 2^(L+1): its layer m is that domain's layer m + 1, whose inverse twiddles
// winv holds (2^(L-1-m) entries).
__device__ __forceinline__ void fr_line_pair(uint32_t* v, uint32_t m, uint32_t j, const uint32_t* __restrict__ winv) {
    const uint32_t a_at = ((j >> m) << (m + 1)) | (j & ((1u << m) - 1)), b_at = a_at + (1u << m);
    uint32_t a = v[a_at], b = v[b_at];
    cm_butterfly<true>(a, b, winv[a_at >> (m + 1)]);
    v[a_at] = a;
    v[b_at] = b;
}

// After the layers, word j of a vector times 2^-L is the coefficient of prod_m pi^m(x)^(bit m of j): natural order.  Word j of
// proof p's four vectors (ev(c): vector c's), scaled, to w; zeros for a masked proof.  The first 2^log_last go to last
// [P][2^log_last][4] in the order rsv_line_eval reads (index bit-reversed over log_last bits); a non-zero one past them
// clears the proof's low-degree flag (fr_draw_one set it).  -> whether j is one of the first.
template <class Ev>
__device__ __forceinline__ bool fr_last_word(Ev ev, uint32_t L, uint32_t log_last, uint64_t p, uint32_t j, bool keep, uint32_t* __restrict__ last,
                                             uint8_t* __restrict__ low, uint32_t* w) {
    const uint32_t scale = L ? 1u << (31 - L) : 1u;  // 2^-L mod P
#pragma unroll
    for (int c = 0; c < 4; c++) w[c] = keep ? m_mul(ev(c), scale) : 0u;
    const bool first = j < (1u << log_last);
    if (first) {
        const uint32_t i = log_last ? bit_reverse(j, log_last) : 0u;
        uint32_t* o = last + ((p << log_last) + i) * 4;
#pragma unroll
        for (int c = 0; c < 4; c++) o[c] = w[c];
    } else if (w[0] | w[1] | w[2] | w[3]) {
        low[p] = 0;
    }
    return first;
}

// The transcript's last step of the stage, by one lane: mix the last polynomial's 2^log_last coefficients (coef(i, k): the
// (i + k)-th of `last`, i even, k 0 or 1) two per mix, a single one at the end of an odd count.  co: the proof's channel.
template <class Coef>
__device__ __forceinline__ void fr_mix_last(uint32_t* co, uint32_t log_last, Coef coef) {
    Channel<0> ch = channel_load(co);
    const uint32_t n = 1u << log_last;
#pragma unroll 1
    for (uint32_t i = 0; i < n; i += 2) {
        const QM31 f = coef(i, 0u);
        if (i + 1 < n) ch.mix_two(f, coef(i, 1u));
        else ch.mix_one(f);
    }
    channel_store(co, ch);
}

// fr_line_pair of layer m of P x 4 vectors of 2^L words (ev [P][4][2^L]), one lane per pair.
__global__ __launch_bounds__(256) void k_fr_line_layer(uint32_t* __restrict__ ev, uint32_t L, uint32_t m, uint32_t P_,
                                                       const uint32_t* __restrict__ winv) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)P_ * 4) << (L - 1)) return;
    const uint64_t row = t >> (L - 1);
    fr_line_pair(ev + (row << L), m, (uint32_t)(t & (((uint64_t)1 << (L - 1)) - 1)), winv);
}

// fr_last_word, one lane per (proof, j): last [P][2^log_last][4], low [P].
__global__ __launch_bounds__(256) void k_fr_last(const uint32_t* __restrict__ ev, uint32_t L, uint32_t log_last, uint32_t P_,
                                                 const uint8_t* __restrict__ mask, uint32_t* __restrict__ last, uint8_t* __restrict__ low) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ((uint64_t)P_ << L)) return;
    const uint64_t p = t >> L;
    const uint32_t j = (uint32_t)(t & (((uint64_t)1 << L) - 1));
    uint32_t w[4];
    fr_last_word([=](int c) { return ev[((p * 4 + c) << L) + j]; }, L, log_last, p, j, !mask || mask[p], last, low, w);
}

// fr_mix_last, one lane per proof: chan [P][16]; a masked proof keeps its zeros.
__global__ __launch_bounds__(64) void k_fr_mix_last(const uint32_t* __restrict__ last, uint32_t log_last, const uint8_t* __restrict__ mask,
                                                    uint32_t P_, uint32_t* __restrict__ chan) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P_ || (mask && !mask[p])) return;
    uint32_t* co = chan + (size_t)p * 16;
    const uint32_t* c = last + ((size_t)p << log_last) * 4;
    fr_mix_last(co, log_last, [=](uint32_t i, uint32_t k) {
        const uint32_t at = 4 * i + 4 * k;
        return q_mk(c[at], c[at + 1], c[at + 2], c[at + 3]);
    });
}

// ---------------------------------------------------------------- the tail form (rsv_fri_commit_tail_dev, tail_log = t)
// One workgroup of 256 lanes per proof finishes what the per-layer form spends a launch per level on: k_fr_tree_top the
// levels t .. 0 of a layer tree and the channel step on its root, k_fr_tail every inner layer of log size <= t and the last
// layer.  Both are loops around the per-layer kernels' own steps — fr_node, fr_draw_one, fr_fold_pair and fr_fold_join,
// fr_line_pair, fr_last_word, fr_mix_last — so every output is the per-layer form's bit for bit.
//
// LDS, word-major as k_fo_subtree's: two node levels ping-ponged, level l in the first 2^T entries when first - l is even
// and in the 2^(T-1) after them when it is odd (48 << T bytes); k_fr_tail also keeps the running evaluation, 4 x 2^T words
// (16 << T bytes).  A level of more than 256 nodes is strided.  Every barrier is reached by the whole workgroup: a masked
// proof is a value (`keep`), not a path.
constexpr uint32_t FR_TAIL_LOG = 10;  // RSV_MAX_FRI_TAIL_LOG
constexpr uint32_t FR_TAIL_NODES = 3u << (FR_TAIL_LOG - 1);

// Where the kept levels of one tree of the pass go (caps == nullptr: nowhere): levels 1 .. c of tree `tree`, proof p0 + p.
struct FrCapOut {
    uint32_t* caps;
    FoCaps at;
    uint32_t tree, c;
    uint64_t p0;
};
// The quotient columns of log size <= FR_TAIL_LOG: bit l of dmask: one of log size l, coordinate j of proof p, value i at
// quot + p * qstride + at[l] + (j << l) + i.
struct FrSmallCols {
    const uint32_t* quot;
    uint64_t qstride;
    uint64_t at[FR_TAIL_LOG + 1];
    uint32_t dmask;
};

// Level l of fr_lds_tree to node[][out ..] and to `kept`, a lane per node; kids(i, a, b): the children of node i.
template <class Data, class Kids>
__device__ __forceinline__ void fr_lds_level(uint32_t (*node)[FR_TAIL_NODES], uint32_t l, bool leaf, uint32_t out, uint32_t* kept, const Data& data,
                                             Kids kids) {
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < (1u << l); i += 256) {
        const Hash8 h = fr_node(leaf, [&](uint32_t* v) { return data(l, i, v); }, [&](Hash8& a, Hash8& b) { kids(i, a, b); });
#pragma unroll
        for (int w = 0; w < 8; w++) node[w][out + i] = h.w[w];
        if (kept) store_hash(kept + (uint64_t)i * 8, h);
    }
}

// Levels first .. 0 of one tree of leaves at `top` >= first, a lane per node.  Level first's children are child [2^(first +
// 1)][8] (top > first) or none (the leaves); data(l, i, v): whether level l carries a column, and node i's four words of it.
// cap(l): where level l is kept, or nullptr.  -> the root, in every lane.  Ends behind a barrier.
template <class Data, class Cap>
__device__ Hash8 fr_lds_tree(uint32_t (*node)[FR_TAIL_NODES], uint32_t top, uint32_t first, const uint32_t* __restrict__ child, Data data, Cap cap) {
#pragma unroll 1
    for (uint32_t l = first + 1; l-- > 0;) {
        const uint32_t out = (first - l) & 1 ? 1u << FR_TAIL_LOG : 0u, in = out ? 0u : 1u << FR_TAIL_LOG;
        // one level loop per source of the children: one callback that branches between the global and the LDS loads compiles
        // to flat loads as a struct and takes the compiler down (a segmentation fault in simplifycfg) as a lambda nested here
        if (l == first && l < top) {
            fr_lds_level(node, l, false, out, cap(l), data, [&](uint32_t i, Hash8& a, Hash8& b) {
                a = load_hash(child + (uint64_t)i * 16);
                b = load_hash(child + (uint64_t)i * 16 + 8);
            });
        } else {
            fr_lds_level(node, l, l == top, out, cap(l), data, [&](uint32_t i, Hash8& a, Hash8& b) {
#pragma unroll
                for (int w = 0; w < 8; w++) {
                    a.w[w] = node[w][in + 2 * i];
                    b.w[w] = node[w][in + 2 * i + 1];
                }
            });
        }
        __syncthreads();
    }
    Hash8 r;
    const uint32_t at = first & 1 ? 1u << FR_TAIL_LOG : 0u;
#pragma unroll
    for (int w = 0; w < 8; w++) r.w[w] = node[w][at];
    return r;
}

__device__ __forceinline__ uint32_t* fr_cap_level(const FrCapOut& k, uint32_t tree, uint32_t c, uint32_t l, uint32_t p) {
    return k.caps && l >= 1 && l <= c ? k.caps + fo_cap_at(k.at, tree, l, k.p0 + p) : nullptr;
}

// The top of layer tree idx of every proof of the pass: levels first = min(top, t) .. 0, then the channel step.  child: level
// first + 1 of the pass, [P][2^(first + 1)][8] (not read when first == top); cols: the columns the levels carry (tree 0).
__global__ __launch_bounds__(256) void k_fr_tree_top(uint32_t top, uint32_t first, const uint32_t* __restrict__ child, FrSmallCols cols,
                                                     FrCapOut cap, FrDraw draw, uint32_t idx) {
    __shared__ uint32_t node[8][FR_TAIL_NODES];
    const uint32_t p = blockIdx.x;
    const uint32_t* q = cols.dmask ? cols.quot + p * cols.qstride : nullptr;
    const Hash8 r = fr_lds_tree(
        node, top, first, first < top ? child + ((uint64_t)p << (first + 1)) * 8 : nullptr,
        [&](uint32_t l, uint32_t i, uint32_t* v) {
            if (!(cols.dmask >> l & 1u)) return false;
            const uint32_t* s = q + cols.at[l] + i;
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = s[(uint64_t)j << l];
            return true;
        },
        [&](uint32_t l) { return fr_cap_level(cap, cap.tree, cap.c, l, p); });
    if (threadIdx.x == 0) fr_draw_one(draw.layer(idx), p, !draw.mask || draw.mask[p], [&] { return r; });
}

// The tail of every proof of the pass: the inner layers of log size l0 .. L + 1 (idx M - l each) and the last layer.
struct FrTail {
    uint32_t M, L, log_last, l0;
    const uint32_t* in;   // the evaluation of log size l0: coordinate j of proof p, value i at in + p * istride + (j << l0) + i
    uint64_t istride;
    uint32_t* layers;     // of the pass's first proof (not read or written when l0 == L)
    uint64_t lstride;
    FrSmallCols cols;     // the columns that join: log sizes l0 .. L + 1
    const uint32_t* inv_x[FR_TAIL_LOG + 1];  // [l], L < l <= l0: 1 / x of the line layer's pairs; [L]: the table of the interpolation
    const uint32_t* inv_y[FR_TAIL_LOG + 1];  // [l], bit l of cols.dmask: 1 / y of the column's pairs
    uint32_t* last_poly;  // of the pass's first proof
};

__global__ __launch_bounds__(256) void k_fr_tail(FrTail a, FrCapOut cap, FrDraw draw) {
    static_assert((1u << (FR_TAIL_LOG - 1)) <= 2 * 256, "a fold keeps two results per lane");
    __shared__ uint32_t node[8][FR_TAIL_NODES];
    __shared__ uint32_t ev[4][1u << FR_TAIL_LOG];
    __shared__ uint32_t s_alpha[4];
    const uint32_t p = blockIdx.x, tid = threadIdx.x;
    const bool keep = !draw.mask || draw.mask[p];
    const auto ev_at = [&](uint32_t i) { return q_mk(ev[0][i], ev[1][i], ev[2][i], ev[3][i]); };
    {
        const uint32_t* s = a.in + p * a.istride;
        for (uint32_t g = tid; g < (4u << a.l0); g += 256) ev[g >> a.l0][g & ((1u << a.l0) - 1)] = s[g];
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t l = a.l0; l > a.L; l--) {
        const uint32_t idx = a.M - l;
        const Hash8 r = fr_lds_tree(
            node, l, l, nullptr,
            [&](uint32_t lv, uint32_t i, uint32_t* v) {
                if (lv != l) return false;
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = ev[j][i];
                return true;
            },
            [&](uint32_t lv) { return fr_cap_level(cap, idx, fo_cap_layers(l, cap.at.h), lv, p); });
        if (tid == 0) {
            const QM31 al = fr_draw_one(draw.layer(idx), p, keep, [&] { return r; });
            s_alpha[0] = al.a.a; s_alpha[1] = al.a.b; s_alpha[2] = al.b.a; s_alpha[3] = al.b.b;
        }
        __syncthreads();
        const QM31 alpha = q_mk(s_alpha[0], s_alpha[1], s_alpha[2], s_alpha[3]);
        const bool join = a.cols.dmask >> l & 1u;
        const uint32_t half = 1u << (l - 1);
        QM31 v[2];
#pragma unroll
        for (int rr = 0; rr < 2; rr++) {
            const uint32_t k = tid + rr * 256;
            v[rr] = q_zero();
            if (k < half && keep) {
                v[rr] = fr_fold_pair(ev_at(2 * k), ev_at(2 * k + 1), a.inv_x[l][k], alpha);
                if (join) {
                    const uint32_t* s = a.cols.quot + p * a.cols.qstride + a.cols.at[l] + 2 * k;
                    v[rr] = fr_fold_join(v[rr], fr_fold_pair(fr_ld(s, l), fr_ld(s + 1, l), a.inv_y[l][k], alpha), alpha);
                }
            }
        }
        __syncthreads();
        // the next layer: where fri_open reads it, unless it is the last evaluation, which no one reads
        uint32_t* d = l - 1 > a.L ? a.layers + p * a.lstride + fr_layer_off(a.M, l - 1) : nullptr;
#pragma unroll
        for (int rr = 0; rr < 2; rr++) {
            const uint32_t k = tid + rr * 256;
            if (k < half) {
                ev[0][k] = v[rr].a.a; ev[1][k] = v[rr].a.b; ev[2][k] = v[rr].b.a; ev[3][k] = v[rr].b.b;
                if (d) fr_st(d + k, l - 1, v[rr]);
            }
        }
        __syncthreads();
    }
    // the last layer; the coefficients stay in ev, in natural order, for the mixes
    const uint32_t L = a.L;
#pragma unroll 1
    for (uint32_t m = 0; m < L; m++) {
        const uint32_t* winv = a.inv_x[L] + cm_tw_off(L + 1, m + 1);
        for (uint32_t g = tid; g < (4u << (L - 1)); g += 256) fr_line_pair(ev[g >> (L - 1)], m, g & ((1u << (L - 1)) - 1), winv);
        __syncthreads();
    }
    for (uint32_t j = tid; j < (1u << L); j += 256) {
        uint32_t w[4];
        if (fr_last_word([&](int c) { return ev[c][j]; }, L, a.log_last, p, j, keep, a.last_poly, draw.low, w)) {
#pragma unroll
            for (int c = 0; c < 4; c++) ev[c][j] = w[c];
        }
    }
    __syncthreads();
    if (tid == 0 && keep)
        fr_mix_last(draw.chan + (size_t)p * 16, a.log_last, [&](uint32_t i, uint32_t k) { return ev_at(a.log_last ? bit_reverse(i + k, a.log_last) : 0u); });
}

// ---------------------------------------------------------------- the recursion circuit's chain (rsv_witness_fri_dev)
// One lane per proof (run_transcript order): mix the 142 sampled values two per mix (the 134 of trees 0..2, then tree
// 3's eight), draw `after`; the three points of the quotients: the OODS point, and it minus the step of CanonicCoset(lp)
// and of CanonicCoset(lq) (k_sp_weights' form).  chan [n][16] read and updated, after [n][4], pts [n][3][8].  A masked
// proof gets zeros in all three.
__global__ __launch_bounds__(64) void k_fr_begin(const uint32_t* __restrict__ samples, const uint32_t* __restrict__ samples3,
                                                 const uint32_t* __restrict__ oods, const uint8_t* __restrict__ mask, uint32_t lp, uint32_t lq,
                                                 uint32_t n, uint32_t* __restrict__ chan, uint32_t* __restrict__ after, uint32_t* __restrict__ pts) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    uint32_t* co = chan + (size_t)p * 16;
    uint32_t* ao = after + (size_t)p * 4;
    uint32_t* po = pts + (size_t)p * 24;
    if (mask && !mask[p]) {
#pragma unroll
        for (int i = 0; i < 16; i++) co[i] = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) ao[i] = 0u;
#pragma unroll
        for (int i = 0; i < 24; i++) po[i] = 0u;
        return;
    }
    Channel<0> ch = channel_load(co);
#pragma unroll 1
    for (uint32_t i = 0; i < 142; i += 2) {
        const uint32_t* s = i < 134 ? samples + ((size_t)p * 134 + i) * 4 : samples3 + ((size_t)p * 8 + (i - 134)) * 4;
        ch.mix(load_hash(s));
    }
    const Hash8 dr = ch.draw();
    channel_store(co, ch);
#pragma unroll
    for (int i = 0; i < 4; i++) ao[i] = dr.w[i];
    const QM31 x = sp_load_q(oods + (size_t)p * 8), y = sp_load_q(oods + (size_t)p * 8 + 4);
    auto put = [&](uint32_t k, QM31 px, QM31 py) {
        uint32_t* o = po + k * 8;
        o[0] = px.a.a; o[1] = px.a.b; o[2] = px.b.a; o[3] = px.b.b;
        o[4] = py.a.a; o[5] = py.a.b; o[6] = py.b.a; o[7] = py.b.b;
    };
    put(0, x, y);
#pragma unroll 1
    for (uint32_t k = 1; k < 3; k++) {
        const uint32_t log = k == 1 ? lp : lq;
        const uint32_t sx = GEN_POW.x[31 - log], sy = GEN_POW.y[31 - log];  // the step's inverse is (sx, -sy)
        put(k, q_add(q_mul_m(x, sx), q_mul_m(y, sy)), q_sub(q_mul_m(y, sx), q_mul_m(x, sy)));
    }
}

}  // namespace rsv
