// fri_api.inc — rsv_fri_sizes, rsv_fri_quotients_dev (the DEEP quotient columns over their whole domains),
// rsv_fri_commit_dev (the FRI layers' trees, the transcript between them, the folds, the last layer's polynomial) and
// rsv_witness_fri_dev (both from the chain's buffers), rsv_fri_cap_sizes and the two forms that also leave the caps of the layer
// trees (rsv_fri_commit_cap_dev, rsv_witness_fri_caps_dev): k_fri.hpp, include/rsv.h.  Included at the end of rsv_hip.hip, after
// composition_api.inc.
//
// Quotients: one quotient column (one LDE log size) at a time; its groups are interpolated (from evaluations) and
// extended block by block with commit_api.inc's streaming helpers, and k_fr_rows consumes each pass of blocks.  Commit: the per-layer form,
// one launch per tree level, one channel launch and one or two fold launches per layer.  With tail_log = t > 0
// (rsv_fri_commit_tail_dev, rsv_witness_fri_tail_dev) the tail form: a tree's levels t .. 0 and its channel step are one launch
// of k_fr_tree_top, and, when the last layer is no larger than 2^t, every inner layer of log size <= t and the last layer are
// one launch of k_fr_tail, a workgroup per proof each.  Same outputs, bit for bit: the kernels of both forms call the same step
// definitions (k_fri.hpp), and the three rsv_fri_commit*_dev entries are one checked path (fri_commit_checked) with zeros for what
// an entry lacks.

namespace {

constexpr size_t FR_MAX_SIZES = RSV_MAX_COMMIT_GROUPS;

// What the points and samples of one group are (rsv::FrGroup's host half).
struct FrSpec {
    const uint32_t* samples;
    uint64_t sstride;
    uint32_t lo[rsv::FR_MAX_POINTS], hi[rsv::FR_MAX_POINTS], entry[rsv::FR_MAX_POINTS], step[rsv::FR_MAX_POINTS];
};

// The distinct log sizes of the groups, descending -> their number.
size_t fr_sizes_of(const rsv_commit_group* g, size_t ng, uint32_t* sizes) {
    size_t ns = 0;
    for (size_t i = 0; i < ng; i++) {
        bool seen = false;
        for (size_t k = 0; k < ns; k++) seen |= sizes[k] == g[i].log_size;
        if (!seen) sizes[ns++] = g[i].log_size;
    }
    std::sort(sizes, sizes + ns, [](uint32_t a, uint32_t b) { return a > b; });
    return ns;
}

struct FrWs {
    uint32_t *coef[rsv::FR_MAX_GROUPS], *ext[rsv::FR_MAX_GROUPS], *par;
};
// Workspace of a pass of P proofs and nb blocks of one quotient column (the groups of log size ls): per group the
// coefficients (from evaluations only) and the extended blocks in flight (one set for a shared group), then the
// constants.
size_t fr_ws_bytes(const rsv_commit_group* g, size_t ng, uint32_t ls, bool interpolate, size_t P, size_t nb, uint32_t par_words, char* base,
                   FrWs* w) {
    rsv::host::Carve sz{base};
    FrWs t{};
    for (size_t i = 0; i < ng; i++) {
        if (g[i].log_size != ls) continue;
        const size_t np = g[i].proof_stride ? P : 1;
        t.coef[i] = interpolate ? sz.take<uint32_t>(np * g[i].n_cols << ls) : nullptr;
        t.ext[i] = sz.take<uint32_t>((np * g[i].n_cols * nb) << ls);
    }
    t.par = sz.take<uint32_t>(P * par_words);
    if (w) *w = t;
    return sz.off;
}

// g / fs: ng <= FR_MAX_GROUPS groups; d_quot: per proof (stride the sum of 4 << (size + b)) the columns in descending size.
int fri_quotients(rsv_ctx* c, const rsv_commit_group* g, const FrSpec* fs, size_t ng, size_t n, uint32_t b, const uint8_t* d_mask, int source,
                  const uint32_t* d_points, uint32_t n_points, const uint32_t* d_after, uint32_t* d_quot) {
    uint32_t sizes[rsv::FR_MAX_GROUPS];
    const size_t ns = fr_sizes_of(g, ng, sizes);
    uint64_t qstride = 0;
    for (size_t s = 0; s < ns; s++) qstride += (uint64_t)4 << (sizes[s] + b);
    if (n == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    const bool interpolate = source == RSV_SAMPLE_COLUMNS;
    hipStream_t st = c->stream;
    uint64_t col_off = 0;
    for (size_t s = 0; s < ns; s++) {
        const uint32_t ls = sizes[s], N = ls + b;
        uint32_t terms = 0;
        for (size_t i = 0; i < ng; i++)
            if (g[i].log_size == ls)
                for (uint32_t k = 0; k < n_points; k++) terms += fs[i].hi[k] > fs[i].lo[k] ? fs[i].hi[k] - fs[i].lo[k] : 0;
        const uint32_t par_words = rsv::FR_TERMS_AT + 4 * terms;
        const auto ws = [&](size_t P, size_t nb, char* base = nullptr, FrWs* w = nullptr) {
            return fr_ws_bytes(g, ng, ls, interpolate, P, nb, par_words, base, w);
        };
        const rsv::host::Pass pass = rsv::host::plan_pass(ws_budget(c), n, (size_t)1 << b, ws);
        const size_t P = pass.P, nb = pass.nb, R = nb << ls;
        for (size_t i = 0; i < ng; i++)
            if (g[i].log_size == ls && !cm_rows_fit((uint64_t)P * g[i].n_cols * nb, ls)) return RSV_E_SIZE;
        if ((uint64_t)P * std::max<size_t>(R / 256, 1) >= CM_GRID_LIM) return RSV_E_SIZE;
        uint32_t rlog = 0;
        while (((size_t)1 << rlog) < R) rlog++;
        // one table per domain: every group of the pass has the size ls
        const uint32_t *tw_inv = nullptr, *tw_fwd;
        int rc = cm_twiddles(c, N, false, &tw_fwd);
        if (rc == RSV_OK && interpolate) rc = cm_twiddles(c, ls, true, &tw_inv);
        FrWs w;
        if (rc == RSV_OK) rc = cm_workspace(c, [&](char* base) { return ws(P, nb, base, &w); });
        if (rc != RSV_OK) return rc;
        for (size_t p0 = 0; p0 < n; p0 += P) {
            const size_t Pc = std::min(P, n - p0);
            rsv::FrRows a{};
            rsv::FrCol& col = a.col;
            const uint32_t* cf[rsv::FR_MAX_GROUPS];
            uint64_t cf_stride[rsv::FR_MAX_GROUPS];
            size_t at[rsv::FR_MAX_GROUPS];
            for (size_t i = 0; i < ng; i++) {
                if (g[i].log_size != ls) continue;
                const uint32_t cols = g[i].n_cols;
                const bool shared = g[i].proof_stride == 0;
                at[col.ng] = i;
                rsv::FrGroup& k = col.g[col.ng++];
                k.ext = w.ext[i];
                k.pstride = shared ? 0 : (uint64_t)cols * R;
                k.samples = fs[i].samples;
                k.sstride = fs[i].sstride;
                k.n_cols = cols;
                for (uint32_t q = 0; q < rsv::FR_MAX_POINTS; q++) {
                    const bool on = q < n_points && fs[i].hi[q] > fs[i].lo[q];
                    k.lo[q] = on ? fs[i].lo[q] : 0;
                    k.hi[q] = on ? fs[i].hi[q] : 0;
                    k.entry[q] = fs[i].entry[q];
                    k.step[q] = fs[i].step[q];
                }
                if (!interpolate) {
                    cf[i] = g[i].d_cols + p0 * g[i].proof_stride;
                    cf_stride[i] = g[i].proof_stride;
                    continue;
                }
                cf[i] = w.coef[i];
                cf_stride[i] = shared ? 0 : (uint64_t)cols << ls;
                cm_interpolate(st, g[i], w.coef[i], p0, Pc, d_mask, true, tw_inv);
            }
            col.np = n_points;
            col.par_words = par_words;
            col.p0 = (uint32_t)p0;
            col.mask = d_mask;
            col.par = w.par;
            hipLaunchKernelGGL(rsv::k_fr_consts, dim3(grid_for(Pc, 64)), dim3(64), 0, st, col, d_points, d_after, (uint32_t)Pc);
            a.rlog = rlog;
            a.N = N;
            a.tw = tw_fwd;
            a.quot = d_quot + p0 * qstride + col_off;
            a.qstride = qstride;
            for (size_t blk0 = 0; blk0 < ((size_t)1 << b); blk0 += nb) {
                // the LDE of blocks blk0 .. blk0 + nb - 1 of every group of this size
                for (uint32_t k = 0; k < col.ng; k++) {
                    const size_t i = at[k];
                    const size_t np = g[i].proof_stride ? Pc : 1;
                    cm_extend(st, g[i], cf[i], cf_stride[i], np * g[i].n_cols, N, nb, blk0, {w.ext[i], (uint64_t)nb << ls}, tw_fwd);
                }
                a.row0 = (uint64_t)blk0 << ls;
                hipLaunchKernelGGL(rsv::k_fr_rows, dim3((unsigned)(Pc * std::max<size_t>(R / 256, 1))), dim3(256), 0, st, a);
            }
        }
        col_off += (uint64_t)4 << N;
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int fr_check_commit(const uint32_t* sizes, size_t ns, uint32_t b, uint32_t log_last, size_t n) {
    if (ns == 0 || ns > FR_MAX_SIZES || b < 1 || b > RSV_MAX_LOG_BLOWUP || n > (1u << 20)) return RSV_E_SIZE;
    if (log_last > RSV_MAX_LOG_LAST_LAYER) return RSV_E_SIZE;
    for (size_t s = 0; s < ns; s++) {
        if (sizes[s] > RSV_MAX_LOG_SIZE || sizes[s] < b + 1 || (s && sizes[s] >= sizes[s - 1])) return RSV_E_SIZE;
        if (sizes[s] - b <= log_last) return RSV_E_SIZE;  // every column is larger than the last layer
    }
    if (sizes[0] - 1 - log_last - b > RSV_MAX_FRI_INNER) return RSV_E_SIZE;
    return RSV_OK;
}

struct FrCommitWs {
    uint32_t *na, *nb, *root, *last;
};
size_t fr_commit_ws_bytes(uint32_t M, uint32_t L, size_t P, char* base, FrCommitWs* w) {
    rsv::host::Carve sz{base};
    FrCommitWs t{};
    t.na = sz.take<uint32_t>((P * 8) << M);
    t.nb = sz.take<uint32_t>((P * 8) << (M - 1));
    t.root = sz.take<uint32_t>(P * 8);
    t.last = sz.take<uint32_t>((P * 4) << L);
    if (w) *w = t;
    return sz.off;
}

// No level of a tree is kept: fr_tree's levels go through the two node buffers.
inline uint32_t* fr_keep_none(uint32_t) { return nullptr; }

// The caps of the layer trees (include/rsv.h: rsv_fri_cap_sizes): tree t, leaves at M - t, keeps its layers 1 .. max(M - t -
// h, 0), each [n][2^l][8], the trees and layers one after another.  -> the words of all; tree_at [1 + n_inner] (may be
// nullptr): the words before tree t.
uint64_t fr_cap_words(uint32_t M, uint32_t n_inner, uint32_t h, uint64_t n, uint64_t* tree_at) {
    uint64_t at = 0;
    for (uint32_t t = 0; t <= n_inner; t++) {
        if (tree_at) tree_at[t] = at;
        at += n * (((uint64_t)16 << rsv::fo_cap_layers(M - t, h)) - 16);
    }
    return at;
}

// One layer tree of a pass of Pc proofs, a launch of k_fr_hash_layer per level top .. last: level l goes to na when top - l
// is even and to nb when it is odd (level 0 to root), and is the next level's children.  data_at(l, &stride): the level's
// column, or nullptr; kept(l): where a level the caller keeps goes instead ([Pc][2^l][8]), or nullptr; after(l, nodes) runs
// behind each level's launch.  fri_commit (last = 0, or tail_log + 1) and fri_open (last = 1) share it.  -> where level `last`
// was left (nullptr when top < last).
template <class DataAt, class Kept, class After>
const uint32_t* fr_tree(hipStream_t st, uint32_t Pc, uint32_t top, uint32_t last, uint32_t* na, uint32_t* nb, uint32_t* root, DataAt data_at, Kept kept,
             After after) {
    const uint32_t* child = nullptr;
    for (uint32_t l = top + 1; l-- > last;) {
        uint64_t dstride = 0;
        const uint32_t* data = data_at(l, &dstride);
        uint32_t* out = l == 0 ? root : ((top - l) & 1 ? nb : na);
        if (uint32_t* k = kept(l)) out = k;
        hipLaunchKernelGGL(rsv::k_fr_hash_layer, dim3(grid_for((size_t)Pc << l, 256)), dim3(256), 0, st, data, dstride, l, Pc, child, out);
        after(l, out);
        child = out;
    }
    return child;
}

// What the commit phase leaves and which form it takes: the arguments of rsv_fri_commit_tail_dev behind d_mask.  sub_log counts
// with d_caps only; tail_log 0: the per-layer form.
struct FrOut {
    uint32_t *d_channel, *d_roots, *d_alphas, *d_layers, *d_last_poly;
    uint8_t* d_low_degree;
    uint32_t sub_log;
    uint32_t* d_caps;
    uint32_t tail_log;
};

int fri_commit(rsv_ctx* c, const uint32_t* d_quot, const uint32_t* sizes, size_t ns, uint32_t b, uint32_t log_last, size_t n,
               const uint8_t* d_mask, const FrOut& o) {
    if (n == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t M = sizes[0], L = log_last + b, n_inner = M - 1 - L, T = o.tail_log, sub_log = o.d_caps ? o.sub_log : 0;
    uint32_t *const d_caps = o.d_caps, *const d_last_poly = o.d_last_poly;
    const bool tail = T && L <= T;  // k_fr_tail takes the inner layers of log size <= T and the last layer
    uint64_t qstride = 0, col_at[FR_MAX_SIZES], lstride = 0;
    for (size_t s = 0; s < ns; s++) {
        col_at[s] = qstride;
        qstride += (uint64_t)4 << sizes[s];
    }
    for (uint32_t i = 0; i < n_inner; i++) lstride += (uint64_t)4 << (M - 1 - i);
    const auto ws = [&](size_t P, size_t, char* base = nullptr, FrCommitWs* w = nullptr) { return fr_commit_ws_bytes(M, L, P, base, w); };
    const size_t P = rsv::host::plan_pass(ws_budget(c), n, 1, ws).P;
    if (((uint64_t)P << M) / 256 >= CM_GRID_LIM) return RSV_E_SIZE;
    // 1 / y of every column's pairs, 1 / x of every inner layer's and of the last layer's interpolation
    const uint32_t *inv_y[FR_MAX_SIZES], *inv_x[RSV_MAX_LOG_SIZE + 2] = {};
    int rc = RSV_OK;
    for (size_t s = 0; s < ns && rc == RSV_OK; s++) rc = cm_twiddles(c, sizes[s], true, &inv_y[s]);
    for (uint32_t l = L; l < M && rc == RSV_OK; l++) rc = cm_twiddles(c, l + 1, true, &inv_x[l]);  // the line domain 2^l
    FrCommitWs w;
    if (rc == RSV_OK) rc = cm_workspace(c, [&](char* base) { return ws(P, 1, base, &w); });
    if (rc != RSV_OK) return rc;
    hipStream_t st = c->stream;
    const uint64_t rstride = (uint64_t)(1 + n_inner) * 8, astride = (uint64_t)(1 + n_inner) * 4;
    rsv::FoCaps caps{d_caps, {}, n, sub_log};
    if (d_caps) fr_cap_words(M, n_inner, sub_log, n, caps.tree_at);
    auto column_of = [&](uint32_t l) -> int {
        for (size_t s = 0; s < ns; s++)
            if (sizes[s] == l) return (int)s;
        return -1;
    };
    rsv::FrSmallCols small{};  // the columns k_fr_tree_top and k_fr_tail read themselves
    const uint32_t* tail_inv_y[rsv::FR_TAIL_LOG + 1] = {};
    for (size_t s = 0; s < ns && T; s++) {
        if (sizes[s] > T) continue;
        small.dmask |= 1u << sizes[s];
        small.at[sizes[s]] = col_at[s];
        tail_inv_y[sizes[s]] = inv_y[s] + rsv::cm_tw_off(sizes[s], 0);
    }
    small.qstride = qstride;
    for (size_t p0 = 0; p0 < n; p0 += P) {
        const uint32_t Pc = (uint32_t)std::min(P, n - p0);
        const uint8_t* mask = d_mask ? d_mask + p0 : nullptr;
        const uint32_t* quot = d_quot + p0 * qstride;
        small.quot = quot;
        uint32_t* chan = o.d_channel + p0 * 16;
        uint32_t* alphas = o.d_alphas + p0 * astride;
        uint32_t* layers = o.d_layers ? o.d_layers + p0 * lstride : nullptr;
        // one tree: the levels top .. 0, `data_at` giving the level's column (or nullptr); the root to w.root.  With d_caps the
        // levels 1 .. c go to the pass's proofs of the cap instead of a node buffer, and are read from there as children.
        // The tail form stops the launches at level T + 1.
        auto tree = [&](uint32_t top, uint32_t stop, auto data_at) -> const uint32_t* {
            const auto none = [](uint32_t, const uint32_t*) {};
            if (!d_caps) return fr_tree(st, Pc, top, stop, w.na, w.nb, w.root, data_at, fr_keep_none, none);
            const uint32_t t = M - top;
            return fr_tree(
                st, Pc, top, stop, w.na, w.nb, w.root, data_at,
                [&](uint32_t l) -> uint32_t* { return l >= 1 && l <= rsv::fo_cap_layers(top, sub_log) ? d_caps + rsv::fo_cap_at(caps, t, l, p0) : nullptr; },
                none);
        };
        const rsv::FrDraw step{mask, chan, o.d_roots + p0 * rstride, rstride, alphas, astride, o.d_low_degree + p0};
        rsv::FrCapOut cap_out{d_caps, caps, 0, 0, p0};
        // tree idx (leaves at top) and the channel step behind it: the per-layer form's launches, or the levels above T and k_fr_tree_top
        auto layer_tree = [&](uint32_t idx, uint32_t top, auto data_at) {
            if (!T) {
                tree(top, 0, data_at);
                const rsv::FrDraw d = step.layer(idx);
                hipLaunchKernelGGL(rsv::k_fr_draw, dim3(grid_for(Pc, 64)), dim3(64), 0, st, w.root, d.mask, Pc, d.chan, d.roots, d.rstride, d.alphas,
                                   d.astride, d.low);
                return;
            }
            const uint32_t* child = top > T ? tree(top, T + 1, data_at) : nullptr;
            cap_out.tree = idx;
            cap_out.c = d_caps ? rsv::fo_cap_layers(top, sub_log) : 0;
            rsv::FrSmallCols cols = small;
            if (idx) cols.dmask = 0;  // an inner tree carries its evaluation at the leaves only, and those are above T
            hipLaunchKernelGGL(rsv::k_fr_tree_top, dim3(Pc), dim3(256), 0, st, top, std::min(top, T), child, cols, cap_out, step, idx);
        };
        // where the running evaluation of log size l lives: inner layer M - 1 - l, or the last evaluation
        auto eval_at = [&](uint32_t l) -> rsv::FrVec {
            if (l == L) return {w.last, (uint64_t)4 << L};
            return {layers + rsv::fr_layer_off(M, l), lstride};
        };
        // the first layer: every quotient column at its own level
        layer_tree(0, M, [&](uint32_t l, uint64_t* stride) -> const uint32_t* {
            const int s = column_of(l);
            *stride = qstride;
            return s < 0 ? nullptr : quot + col_at[s];
        });
        {
            const rsv::FrVec src{const_cast<uint32_t*>(quot), qstride};
            hipLaunchKernelGGL(rsv::k_fr_fold<false>, dim3(grid_for((size_t)Pc << (M - 1), 256)), dim3(256), 0, st, src, eval_at(M - 1), M, Pc,
                               inv_y[0] + rsv::cm_tw_off(M, 0), alphas, astride, mask);
        }
        for (uint32_t i = 0; i < n_inner; i++) {
            const uint32_t l = M - 1 - i;
            if (tail && l <= T) break;
            const rsv::FrVec cur = eval_at(l), next = eval_at(l - 1);
            layer_tree(i + 1, l, [&](uint32_t lv, uint64_t* stride) -> const uint32_t* {
                *stride = cur.stride;
                return lv == l ? cur.base : nullptr;
            });
            const dim3 grid(grid_for((size_t)Pc << (l - 1), 256));
            hipLaunchKernelGGL(rsv::k_fr_fold<false>, grid, dim3(256), 0, st, cur, next, l, Pc, inv_x[l] + rsv::cm_tw_off(l + 1, 1), alphas + (i + 1) * 4,
                               astride, mask);
            const int s = column_of(l);
            if (s >= 0) {
                const rsv::FrVec src{const_cast<uint32_t*>(quot) + col_at[s], qstride};
                hipLaunchKernelGGL(rsv::k_fr_fold<true>, grid, dim3(256), 0, st, src, next, l, Pc, inv_y[s] + rsv::cm_tw_off(l, 0), alphas + (i + 1) * 4,
                                   astride, mask);
            }
        }
        if (tail) {
            // the evaluation the folds above left, of log size min(T, M - 1), through its layers and the last layer
            rsv::FrTail a{};
            a.M = M, a.L = L, a.log_last = log_last, a.l0 = std::min(T, M - 1);
            const rsv::FrVec in = eval_at(a.l0);
            a.in = in.base, a.istride = in.stride, a.layers = layers, a.lstride = lstride;
            a.cols = small;
            a.cols.dmask &= (2u << a.l0) - 1;
            for (uint32_t l = L; l <= a.l0; l++) {
                a.inv_x[l] = l == L ? inv_x[l] : inv_x[l] + rsv::cm_tw_off(l + 1, 1);
                a.inv_y[l] = tail_inv_y[l];
            }
            a.last_poly = d_last_poly + ((p0 * 4) << log_last);
            hipLaunchKernelGGL(rsv::k_fr_tail, dim3(Pc), dim3(256), 0, st, a, cap_out, step);
            continue;
        }
        // the last layer: the evaluation's coefficients, the first 2^log_last out, the rest checked, the final mixes
        for (uint32_t m = 0; m < L; m++)
            hipLaunchKernelGGL(rsv::k_fr_line_layer, dim3(grid_for(((size_t)Pc * 4) << (L - 1), 256)), dim3(256), 0, st, w.last, L, m, Pc,
                               inv_x[L] + rsv::cm_tw_off(L + 1, m + 1));
        hipLaunchKernelGGL(rsv::k_fr_last, dim3(grid_for((size_t)Pc << L, 256)), dim3(256), 0, st, w.last, L, log_last, Pc, mask,
                           d_last_poly + ((p0 * 4) << log_last), o.d_low_degree + p0);
        hipLaunchKernelGGL(rsv::k_fr_mix_last, dim3(grid_for(Pc, 64)), dim3(64), 0, st, d_last_poly + ((p0 * 4) << log_last), log_last, mask, Pc,
                           chan);
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int fr_check_chain(uint32_t lp, uint32_t lq, uint32_t b, uint32_t log_last, size_t n, uint32_t* sizes, size_t* ns) {
    int rc = co_check_sizes(lp, lq, n);
    if (rc != RSV_OK) return rc;
    if (b < 1 || b > RSV_MAX_LOG_BLOWUP) return RSV_E_SIZE;
    const uint32_t M = co_clb(lp, lq) - 1 + b, A = lp + b, B = lq + b;
    if (M > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;
    size_t k = 0;
    sizes[k++] = M;
    sizes[k++] = std::max(A, B);
    if (A != B) sizes[k++] = std::min(A, B);
    *ns = k;
    return fr_check_commit(sizes, k, b, log_last, n);
}

// The one checked path of rsv_fri_commit_dev, rsv_fri_commit_cap_dev and rsv_fri_commit_tail_dev: what the first refuses, with
// d_caps what the second adds, then the third's bound, in that order.
int fri_commit_checked(rsv_ctx* c, const uint32_t* d_quot, const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup, uint32_t log_last, size_t n,
                       const uint8_t* d_mask, const FrOut& o) {
    if (!c || !d_quot || !sizes || !o.d_channel || !o.d_roots || !o.d_alphas || !o.d_last_poly || !o.d_low_degree) return RSV_E_NULL;
    const int rc = fr_check_commit(sizes, n_sizes, log_blowup, log_last, n);
    if (rc != RSV_OK) return rc;
    if (!o.d_layers && sizes[0] - 1 - log_last - log_blowup > 0) return RSV_E_NULL;
    if (o.d_caps && (o.sub_log < 1 || o.sub_log > RSV_MAX_FRI_SUB_LOG)) return RSV_E_SIZE;
    if (((uintptr_t)d_quot & 3) || ((uintptr_t)o.d_channel & 3) || ((uintptr_t)o.d_roots & 3) || ((uintptr_t)o.d_alphas & 3) ||
        ((uintptr_t)o.d_layers & 3) || ((uintptr_t)o.d_last_poly & 3) || ((uintptr_t)o.d_caps & 3))
        return RSV_E_SIZE;
    if (o.tail_log > RSV_MAX_FRI_TAIL_LOG) return RSV_E_SIZE;
    return fri_commit(c, d_quot, sizes, n_sizes, log_blowup, log_last, n, d_mask, o);
}

}  // namespace

extern "C" {

int rsv_fri_sizes(uint32_t lp, uint32_t lq, uint32_t log_blowup, uint32_t log_last, uint32_t* sizes, uint32_t* n_sizes, uint32_t* n_inner,
                  size_t* quot_words, size_t* layer_words, size_t* last_words) {
    if (!sizes || !n_sizes || !n_inner || !quot_words || !layer_words || !last_words) return RSV_E_NULL;
    uint32_t sz[3];
    size_t ns = 0;
    const int rc = fr_check_chain(lp, lq, log_blowup, log_last, 0, sz, &ns);
    if (rc != RSV_OK) return rc;
    size_t q = 0, lw = 0;
    for (size_t s = 0; s < ns; s++) {
        sizes[s] = sz[s];
        q += (size_t)4 << sz[s];
    }
    const uint32_t ni = sz[0] - 1 - log_last - log_blowup;
    for (uint32_t i = 0; i < ni; i++) lw += (size_t)4 << (sz[0] - 1 - i);
    *n_sizes = (uint32_t)ns;
    *n_inner = ni;
    *quot_words = q;
    *layer_words = lw;
    *last_words = (size_t)4 << log_last;
    return RSV_OK;
}

int rsv_fri_quotients_dev(rsv_ctx* c, const rsv_commit_group* groups, const rsv_fri_group_points* group_points, size_t n_groups, size_t n,
                          uint32_t log_blowup, const uint8_t* d_mask, int source, const uint32_t* d_points, uint32_t n_points,
                          const uint32_t* d_samples, const uint32_t* d_after, uint32_t* d_quot) {
    if (!c || !groups || !group_points || !d_points || !d_samples || !d_after || !d_quot) return RSV_E_NULL;
    if (n_points < 1 || n_points > RSV_MAX_SAMPLE_POINTS || n_groups == 0 || n_groups > RSV_MAX_COMMIT_GROUPS || n > (1u << 20)) return RSV_E_SIZE;
    if (log_blowup < 1 || log_blowup > RSV_MAX_LOG_BLOWUP) return RSV_E_SIZE;
    if (source != RSV_SAMPLE_COLUMNS && source != RSV_SAMPLE_COEFFS) return RSV_E_SIZE;
    if (((uintptr_t)d_points & 3) || ((uintptr_t)d_samples & 3) || ((uintptr_t)d_after & 3) || ((uintptr_t)d_quot & 3)) return RSV_E_SIZE;
    uint64_t total = 0;
    for (size_t i = 0; i < n_groups; i++) {
        if (!groups[i].d_cols) return RSV_E_NULL;
        if (groups[i].n_cols == 0 || groups[i].log_size < 1 || groups[i].log_size + log_blowup > RSV_MAX_LOG_SIZE || ((uintptr_t)groups[i].d_cols & 3))
            return RSV_E_SIZE;
        for (uint32_t k = 0; k < n_points; k++)
            if (group_points[i].col_hi[k] > groups[i].n_cols) return RSV_E_SIZE;
        total += groups[i].n_cols;
    }
    if (total * n_points > 0x3fffffffu) return RSV_E_SIZE;
    FrSpec fs[RSV_MAX_COMMIT_GROUPS];
    uint32_t col0 = 0;
    for (size_t i = 0; i < n_groups; i++) {
        fs[i].samples = d_samples;
        fs[i].sstride = (uint64_t)n_points * total * 4;
        for (uint32_t k = 0; k < rsv::FR_MAX_POINTS; k++) {
            const bool on = k < n_points;
            fs[i].lo[k] = on ? group_points[i].col_lo[k] : 0;
            fs[i].hi[k] = on ? group_points[i].col_hi[k] : 0;
            fs[i].entry[k] = (uint32_t)(k * total) + col0 + fs[i].lo[k];
            fs[i].step[k] = 1;
        }
        col0 += groups[i].n_cols;
    }
    return fri_quotients(c, groups, fs, n_groups, n, log_blowup, d_mask, source, d_points, n_points, d_after, d_quot);
}

int rsv_fri_commit_dev(rsv_ctx* c, const uint32_t* d_quot, const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup, uint32_t log_last, size_t n,
                       const uint8_t* d_mask, uint32_t* d_channel, uint32_t* d_roots, uint32_t* d_alphas, uint32_t* d_layers,
                       uint32_t* d_last_poly, uint8_t* d_low_degree) {
    return fri_commit_checked(c, d_quot, sizes, n_sizes, log_blowup, log_last, n, d_mask,
                              {d_channel, d_roots, d_alphas, d_layers, d_last_poly, d_low_degree, 0, nullptr, 0});
}

int rsv_fri_cap_sizes(const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup, uint32_t log_last, uint32_t sub_log, size_t n, size_t* cap_words,
                      size_t* tree_words) {
    if (!sizes || !cap_words) return RSV_E_NULL;
    const int rc = fr_check_commit(sizes, n_sizes, log_blowup, log_last, n);
    if (rc != RSV_OK) return rc;
    if (sub_log < 1 || sub_log > RSV_MAX_FRI_SUB_LOG) return RSV_E_SIZE;
    const uint32_t n_inner = sizes[0] - 1 - log_last - log_blowup;
    uint64_t at[rsv::FO_MAX_TREES];
    *cap_words = (size_t)fr_cap_words(sizes[0], n_inner, sub_log, n, at);
    for (uint32_t t = 0; tree_words && t <= n_inner; t++) tree_words[t] = (size_t)at[t];
    return RSV_OK;
}

int rsv_fri_commit_cap_dev(rsv_ctx* c, const uint32_t* d_quot, const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup, uint32_t log_last,
                           size_t n, const uint8_t* d_mask, uint32_t* d_channel, uint32_t* d_roots, uint32_t* d_alphas, uint32_t* d_layers,
                           uint32_t* d_last_poly, uint8_t* d_low_degree, uint32_t sub_log, uint32_t* d_caps) {
    return fri_commit_checked(c, d_quot, sizes, n_sizes, log_blowup, log_last, n, d_mask,
                              {d_channel, d_roots, d_alphas, d_layers, d_last_poly, d_low_degree, sub_log, d_caps, 0});
}

int rsv_fri_commit_tail_dev(rsv_ctx* c, const uint32_t* d_quot, const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup, uint32_t log_last,
                            size_t n, const uint8_t* d_mask, uint32_t* d_channel, uint32_t* d_roots, uint32_t* d_alphas, uint32_t* d_layers,
                            uint32_t* d_last_poly, uint8_t* d_low_degree, uint32_t sub_log, uint32_t* d_caps, uint32_t tail_log) {
    return fri_commit_checked(c, d_quot, sizes, n_sizes, log_blowup, log_last, n, d_mask,
                              {d_channel, d_roots, d_alphas, d_layers, d_last_poly, d_low_degree, sub_log, d_caps, tail_log});
}

}  // extern "C"

namespace {

// rsv_witness_fri_dev; with d_caps, rsv_witness_fri_caps_dev; with tail_log, rsv_witness_fri_tail_dev.
int witness_fri(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon, const uint32_t* d_ops,
                const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept, const uint8_t* d_ok, size_t n,
                uint32_t log_blowup, uint32_t log_last, const uint32_t* d_comp, const uint32_t* d_oods, const uint32_t* d_samples,
                const uint32_t* d_samples3, uint32_t* d_after, uint32_t* d_quot, const FrOut& o) {
    const ChainArgs a{c, prog, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, d_ok, n, log_blowup};
    uint32_t* const d_channel = o.d_channel;
    if (chain_null(a, d_comp, d_oods, d_samples, d_samples3, d_channel, d_after, d_quot, o.d_roots, o.d_alphas, o.d_last_poly, o.d_low_degree))
        return RSV_E_NULL;
    if (chain_misaligned(a, d_comp, d_oods, d_samples, d_samples3, d_channel, d_after, d_quot, o.d_roots, o.d_alphas, o.d_layers, o.d_last_poly))
        return RSV_E_SIZE;
    if (o.d_caps && (o.sub_log < 1 || o.sub_log > RSV_MAX_FRI_SUB_LOG || ((uintptr_t)o.d_caps & 3))) return RSV_E_SIZE;
    if (prog->gates.empty()) return RSV_E_SIZE;  // built programs only
    const uint32_t lp = prog->trace_lp, lq = prog->trace_lq;
    uint32_t sizes[3];
    size_t ns = 0;
    int rc = fr_check_chain(lp, lq, log_blowup, log_last, n, sizes, &ns);
    if (rc != RSV_OK) return rc;
    // A proof for the verifier: a column enters the fold in front of the inner layer of half its size (the reference's prover
    // asserts that every column met one; its verifier folds nothing in behind the last inner layer).  The smallest column one
    // size above the last layer would go into the last polynomial alone, and no verifier accepts that proof (RSV_R_FRI_LAST).
    // rsv_fri_sizes stays the arithmetic of the sizes and answers there.
    if (sizes[ns - 1] - log_blowup == log_last + 1) return RSV_E_SIZE;
    if (!o.d_layers && sizes[0] - 1 - log_last - log_blowup > 0) return RSV_E_NULL;
    if (o.tail_log > RSV_MAX_FRI_TAIL_LOG) return RSV_E_SIZE;
    ChainTrees ct;
    rc = chain_open(a, &ct);
    if (rc != RSV_OK || n == 0) return rc;
    const uint8_t* mask = ct.mask;
    rc = ensure_buf(c, &c->ws_fri, &c->ws_fri_bytes, n * 24 * 4);
    if (rc != RSV_OK) return rc;
    uint32_t* pts = static_cast<uint32_t*>(c->ws_fri);
    hipLaunchKernelGGL(rsv::k_fr_begin, dim3(grid_for(n, 64)), dim3(64), 0, c->stream, d_samples, d_samples3, d_oods, mask, lp, lq, (uint32_t)n,
                       d_channel, d_after, pts);
    // The quotient columns' groups: tree 3, then the groups of CHAIN_SAMPLES (per tree the Plonk groups and the Poseidon
    // groups: one column where the sizes are equal).  Points: 0 the OODS point, 1 and 2 it minus the step of lp / lq.
    rsv_commit_group g[rsv::FR_MAX_GROUPS];
    FrSpec fs[rsv::FR_MAX_GROUPS] = {};
    size_t ng = 0;
    auto add = [&](const rsv_commit_group& grp, const uint32_t* samples, uint64_t sstride, uint32_t entry, uint32_t step, uint32_t prev_point) {
        g[ng] = grp;
        fs[ng].samples = samples;
        fs[ng].sstride = sstride;
        fs[ng].lo[0] = 0;
        fs[ng].hi[0] = grp.n_cols;
        fs[ng].entry[0] = entry;
        fs[ng].step[0] = step;
        if (prev_point) {
            fs[ng].hi[prev_point] = grp.n_cols;
            fs[ng].entry[prev_point] = entry - 1;
            fs[ng].step[prev_point] = step;
        }
        ng++;
    };
    const uint32_t L3 = co_clb(lp, lq) - 1;
    add({L3, 8, d_comp, (uint64_t)8 << L3, nullptr, nullptr}, d_samples3, 32, 0, 1, 0);
    for (const ChainSamples& s : CHAIN_SAMPLES) {
        const rsv_commit_group& t = ct.tree(s.tree)[s.group];
        add({t.log_size, s.cols, t.d_cols + ((size_t)s.col0 << t.log_size), t.proof_stride, nullptr, nullptr}, d_samples,
            CHAIN_SAMPLE_VALUES * 4, s.entry, s.step, s.prev_point);
    }
    rc = fri_quotients(c, g, fs, ng, n, log_blowup, mask, RSV_SAMPLE_COLUMNS, pts, 3, d_after, d_quot);
    if (rc != RSV_OK) return rc;
    return fri_commit(c, d_quot, sizes, ns, log_blowup, log_last, n, mask, o);
}

}  // namespace

extern "C" {

int rsv_witness_fri_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon, const uint32_t* d_ops,
                        const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept, const uint8_t* d_ok, size_t n,
                        uint32_t log_blowup, uint32_t log_last, const uint32_t* d_comp, const uint32_t* d_oods, const uint32_t* d_samples,
                        const uint32_t* d_samples3, uint32_t* d_channel, uint32_t* d_after, uint32_t* d_quot, uint32_t* d_roots,
                        uint32_t* d_alphas, uint32_t* d_layers, uint32_t* d_last_poly, uint8_t* d_low_degree) {
    return witness_fri(c, prog, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, d_ok, n, log_blowup, log_last, d_comp, d_oods,
                       d_samples, d_samples3, d_after, d_quot, {d_channel, d_roots, d_alphas, d_layers, d_last_poly, d_low_degree, 0, nullptr, 0});
}

int rsv_witness_fri_caps_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                             const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept,
                             const uint8_t* d_ok, size_t n, uint32_t log_blowup, uint32_t log_last, const uint32_t* d_comp, const uint32_t* d_oods,
                             const uint32_t* d_samples, const uint32_t* d_samples3, uint32_t* d_channel, uint32_t* d_after, uint32_t* d_quot,
                             uint32_t* d_roots, uint32_t* d_alphas, uint32_t* d_layers, uint32_t* d_last_poly, uint8_t* d_low_degree,
                             uint32_t sub_log, uint32_t* d_caps) {
    return witness_fri(c, prog, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, d_ok, n, log_blowup, log_last, d_comp, d_oods,
                       d_samples, d_samples3, d_after, d_quot, {d_channel, d_roots, d_alphas, d_layers, d_last_poly, d_low_degree, sub_log, d_caps, 0});
}

int rsv_witness_fri_tail_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                             const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept,
                             const uint8_t* d_ok, size_t n, uint32_t log_blowup, uint32_t log_last, const uint32_t* d_comp, const uint32_t* d_oods,
                             const uint32_t* d_samples, const uint32_t* d_samples3, uint32_t* d_channel, uint32_t* d_after, uint32_t* d_quot,
                             uint32_t* d_roots, uint32_t* d_alphas, uint32_t* d_layers, uint32_t* d_last_poly, uint8_t* d_low_degree,
                             uint32_t sub_log, uint32_t* d_caps, uint32_t tail_log) {
    return witness_fri(c, prog, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, d_ok, n, log_blowup, log_last, d_comp, d_oods,
                       d_samples, d_samples3, d_after, d_quot, {d_channel, d_roots, d_alphas, d_layers, d_last_poly, d_low_degree, sub_log, d_caps, tail_log});
}

}  // extern "C"
