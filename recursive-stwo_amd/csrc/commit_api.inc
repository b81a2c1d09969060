// commit_api.inc — rsv_commit_tree_dev / rsv_commit_tree_cap_dev (a generic tree commitment: interpolation, LDE, mixed-size
// Merkle tree, optionally leaving the tree's cap) and rsv_witness_commit_dev / rsv_witness_commit_caps_dev /
// rsv_witness_commit (trees 0, 1, 2 of the recursion circuit's next proof and the transcript draws between them):
// k_commit.hpp, include/rsv.h.  Included at the end of rsv_hip.hip, after interaction_api.inc; decommit_api.inc follows.
//
// Also the home of what every stage that takes groups of columns shares (decommit, sample, composition and fri_api.inc
// after it): the twiddle tables, the FFT launches and the streaming helpers below them.  commit_tree is their first user.

namespace {

// The twiddle table of the domain 2^N (inverse: of the interpolation), computed on the context's stream once.
int cm_twiddles(rsv_ctx* c, uint32_t N, bool inverse, const uint32_t** out) {
    uint32_t*& t = c->cm_tw[inverse ? 1 : 0][N];
    if (!t) {
        const size_t words = ((size_t)1 << N) - 1;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t), std::max<size_t>(words, 1) * 4));
        if (words) hipLaunchKernelGGL(rsv::k_cm_twiddles, dim3(grid_for(words, 256)), dim3(256), 0, c->stream, t, N, inverse ? 1u : 0u);
        HIP_TRY(hipGetLastError());
    }
    *out = t;
    return RSV_OK;
}

// Every butterfly layer of a set of rows: interpolation (INV: layers ascending, the first pass reading src) or the forward
// FFT of the blocks (descending, the first pass reading the coefficients).
template <bool INV>
void cm_fft(hipStream_t st, const rsv::CmRows& r, const rsv::CmSrc& s, const uint32_t* tw) {
    const uint32_t c = std::min(r.log, rsv::CM_LDS_LOG);
    const rsv::CmSrc none{};
    const uint64_t pairs = r.rows << (r.log ? r.log - 1 : 0);
    const dim3 lds_grid((unsigned)(r.rows << (r.log - c)));
    if (INV) {
        hipLaunchKernelGGL(rsv::k_cm_fft_lds<true>, lds_grid, dim3(256), 0, st, r, s, tw, c);
        for (uint32_t m = c; m < r.log; m++) hipLaunchKernelGGL(rsv::k_cm_fft_layer<true>, dim3(grid_for(pairs, 256)), dim3(256), 0, st, r, none, tw, m);
    } else {
        for (uint32_t m = r.log; m-- > c;)
            hipLaunchKernelGGL(rsv::k_cm_fft_layer<false>, dim3(grid_for(pairs, 256)), dim3(256), 0, st, r, m + 1 == r.log ? s : none, tw, m);
        hipLaunchKernelGGL(rsv::k_cm_fft_lds<false>, lds_grid, dim3(256), 0, st, r, r.log > c ? none : s, tw, c);
    }
}

// ---- The streaming of column groups (rsv_commit_group) that commit_tree, decommit_tree, sample_groups, composition and
// fri_quotients share.  A driver sizes a pass with rsv::host::plan_pass over its own *_ws_bytes, tests cm_rows_fit per
// group and the limits of its own launches, looks the tables up, carves its workspace with cm_workspace, and per pass calls
// cm_interpolate and then, per range of blocks, cm_extend (the block-list form: cm_extension and dc_fft).

constexpr uint64_t CM_GRID_LIM = (uint64_t)1 << 31;  // every launch's grid stays below 2^31 workgroups

// The FFT launches over `rows` rows of 2^log words stay below the limit (a row per workgroup, or 256 words).
bool cm_rows_fit(uint64_t rows, uint32_t log) { return rows < CM_GRID_LIM && (rows << log) / 256 < CM_GRID_LIM; }

// Per group the inverse table of its size (tw_inv; nullptr for a coefficient source) and the forward table of its LDE
// domain 2^(log_size + b) (tw_fwd; nullptr where the driver extends to a domain of its own).
int cm_group_twiddles(rsv_ctx* c, const rsv_commit_group* g, size_t ng, uint32_t b, const uint32_t** tw_inv, const uint32_t** tw_fwd) {
    int rc = RSV_OK;
    for (size_t i = 0; i < ng && rc == RSV_OK; i++) {
        if (tw_inv) rc = cm_twiddles(c, g[i].log_size, true, &tw_inv[i]);
        if (tw_fwd && rc == RSV_OK) rc = cm_twiddles(c, g[i].log_size + b, false, &tw_fwd[i]);
    }
    return rc;
}

// The context's pass workspace, large enough for layout(nullptr) bytes, then carved by layout(its base).
template <class Layout>
int cm_workspace(rsv_ctx* c, Layout layout) {
    const int rc = ensure_buf(c, &c->ws_commit, &c->ws_commit_bytes, layout(nullptr));
    if (rc == RSV_OK) layout(static_cast<char*>(c->ws_commit));
    return rc;
}

// Interpolation: the columns of proofs p0 .. p0 + Pc - 1 -> the coefficients at dst, masked proofs zero.  With `once`, a
// group that every proof shares (proof_stride == 0) is held once, unmasked, and only the first pass makes it.
void cm_interpolate(hipStream_t st, const rsv_commit_group& g, uint32_t* dst, size_t p0, size_t Pc, const uint8_t* d_mask, bool once,
                    const uint32_t* tw) {
    const bool shared = once && g.proof_stride == 0;
    if (shared && p0) return;
    const uint32_t log = g.log_size;
    const size_t row = (size_t)1 << log;
    const rsv::CmRows r{dst, row, (uint64_t)(shared ? 1 : Pc) * g.n_cols, log, log, 1, 0};
    const rsv::CmSrc s{g.d_cols + p0 * g.proof_stride, g.proof_stride, row, shared ? nullptr : d_mask, g.n_cols, (uint32_t)p0,
                       log ? 1u << (31 - log) : 1u};  // 2^-log = 2^(31-log) mod P
    cm_fft<true>(st, r, s, tw);
}

// Where a group's blocks in flight are: those of (proof, column) row pc from base + pc * pc_stride on.
struct CmBlocks {
    uint32_t* base;
    uint64_t pc_stride;
};
// The extension of `pcs` (proof, column) rows of a group, their coefficients at coef with pstride words between two
// proofs, to blocks blk0 .. blk0 + nb - 1 (2^log_size rows each) of the domain 2^N.
struct CmExt {
    rsv::CmRows r;
    rsv::CmSrc s;
};
CmExt cm_extension(const rsv_commit_group& g, const uint32_t* coef, uint64_t pstride, uint64_t pcs, uint32_t N, size_t nb, size_t blk0,
                   CmBlocks to) {
    const uint32_t log = g.log_size;
    return {{to.base, to.pc_stride, pcs * nb, log, N, (uint32_t)nb, (uint32_t)blk0}, {coef, pstride, (uint64_t)1 << log, nullptr, g.n_cols, 0, 1}};
}
void cm_extend(hipStream_t st, const rsv_commit_group& g, const uint32_t* coef, uint64_t pstride, uint64_t pcs, uint32_t N, size_t nb,
               size_t blk0, CmBlocks to, const uint32_t* tw) {
    const CmExt e = cm_extension(g, coef, pstride, pcs, N, nb, blk0, to);
    cm_fft<false>(st, e.r, e.s, tw);
}

// Level l of the block subtrees of a pass of Pc proofs and nb blocks: the groups whose LDE lives there, in commitment
// order, their blocks at at[i].  The caller adds child, out and (commit_tree) blk0.
rsv::CmHashArgs cm_layer_args(const rsv_commit_group* g, size_t ng, uint32_t b, uint32_t l, const CmBlocks* at, size_t Pc, size_t nb) {
    rsv::CmHashArgs a{};
    a.lw = l - b;
    a.nb = (uint32_t)nb;
    a.P = (uint32_t)Pc;
    a.b = b;
    for (size_t i = 0; i < ng; i++) {
        if (g[i].log_size + b != l) continue;
        a.g[a.ng++] = {at[i].base, at[i].pc_stride, g[i].n_cols};
        a.n_cols += g[i].n_cols;
    }
    return a;
}

struct CmWs {
    uint32_t *coef[RSV_MAX_COMMIT_GROUPS], *lde[RSV_MAX_COMMIT_GROUPS], *na, *nbuf, *broots, *ta, *tb;
};

// Workspace of a pass of P proofs and nb blocks (bytes, with Carve's alignment); with w, also where each part goes.
size_t cm_ws_bytes(const rsv_commit_group* g, size_t ng, uint32_t b, uint32_t Lmax, size_t P, size_t nb, char* base, CmWs* w) {
    rsv::host::Carve sz{base};
    CmWs t{};
    for (size_t i = 0; i < ng; i++) {
        const size_t row = (size_t)1 << g[i].log_size;
        t.coef[i] = g[i].d_coeffs ? nullptr : sz.take<uint32_t>(P * g[i].n_cols * row);
        t.lde[i] = g[i].d_lde ? nullptr : sz.take<uint32_t>(P * g[i].n_cols * nb * row);
    }
    const size_t leaves = P * nb << (Lmax - b);
    t.na = sz.take<uint32_t>(leaves * 8);
    t.nbuf = sz.take<uint32_t>(std::max<size_t>(leaves / 2, 1) * 8);
    t.broots = sz.take<uint32_t>((P << b) * 8);
    t.ta = sz.take<uint32_t>((P << (b - 1)) * 8);
    t.tb = sz.take<uint32_t>((P << (b - 1)) * 8);
    if (w) *w = t;
    return sz.off;
}

// d_cap (may be nullptr): the nodes of layers 0 .. b of proof i in heap order at d_cap + i * cap_stride (words).
int commit_tree(rsv_ctx* c, const rsv_commit_group* g, size_t ng, size_t n, uint32_t b, const uint8_t* d_mask, uint32_t* d_roots,
                uint32_t roots_stride, uint32_t* d_cap = nullptr, uint64_t cap_stride = 0) {
    if (!c || !g || !d_roots) return RSV_E_NULL;
    if (ng == 0 || ng > RSV_MAX_COMMIT_GROUPS || n > (1u << 20) || b < 1 || b > RSV_MAX_LOG_BLOWUP) return RSV_E_SIZE;
    if (((uintptr_t)d_roots & 3) || ((uintptr_t)d_cap & 3)) return RSV_E_SIZE;
    uint32_t Lmax = 0;
    for (size_t i = 0; i < ng; i++) {
        if (!g[i].d_cols) return RSV_E_NULL;
        if (g[i].n_cols == 0 || g[i].log_size + b > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;
        if (((uintptr_t)g[i].d_cols & 3) || ((uintptr_t)g[i].d_coeffs & 3) || ((uintptr_t)g[i].d_lde & 3)) return RSV_E_SIZE;
        Lmax = std::max(Lmax, g[i].log_size + b);
    }
    if (n == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    const auto ws = [&](size_t P, size_t nb, char* base = nullptr, CmWs* w = nullptr) { return cm_ws_bytes(g, ng, b, Lmax, P, nb, base, w); };
    const rsv::host::Pass pass = rsv::host::plan_pass(ws_budget(c), n, (size_t)1 << b, ws);
    const size_t P = pass.P, nb = pass.nb;
    for (size_t i = 0; i < ng; i++)
        if (!cm_rows_fit((uint64_t)P * g[i].n_cols * nb, g[i].log_size)) return RSV_E_SIZE;
    if (((uint64_t)P * nb << (Lmax - b)) / 256 >= CM_GRID_LIM) return RSV_E_SIZE;
    const uint32_t *tw_inv[RSV_MAX_COMMIT_GROUPS], *tw_fwd[RSV_MAX_COMMIT_GROUPS];
    int rc = cm_group_twiddles(c, g, ng, b, tw_inv, tw_fwd);
    CmWs w;
    if (rc == RSV_OK) rc = cm_workspace(c, [&](char* base) { return ws(P, nb, base, &w); });
    if (rc != RSV_OK) return rc;
    hipStream_t st = c->stream;
    for (size_t p0 = 0; p0 < n; p0 += P) {
        const size_t Pc = std::min(P, n - p0);
        // the coefficients, in d_coeffs or the workspace
        const uint32_t* cf[RSV_MAX_COMMIT_GROUPS];
        for (size_t i = 0; i < ng; i++) {
            uint32_t* dst = g[i].d_coeffs ? g[i].d_coeffs + (p0 * g[i].n_cols << g[i].log_size) : w.coef[i];
            cm_interpolate(st, g[i], dst, p0, Pc, d_mask, false, tw_inv[i]);
            cf[i] = dst;
        }
        for (size_t blk0 = 0; blk0 < ((size_t)1 << b); blk0 += nb) {
            // the LDE of blocks blk0 .. blk0 + nb - 1, in d_lde or the workspace
            CmBlocks at[RSV_MAX_COMMIT_GROUPS];
            for (size_t i = 0; i < ng; i++) {
                const uint32_t log = g[i].log_size, cols = g[i].n_cols, N = log + b;
                if (g[i].d_lde) at[i] = {g[i].d_lde + p0 * cols * ((size_t)1 << N) + (blk0 << log), (uint64_t)1 << N};
                else at[i] = {w.lde[i], (uint64_t)nb << log};
                cm_extend(st, g[i], cf[i], (uint64_t)cols << log, (uint64_t)Pc * cols, N, nb, blk0, at[i], tw_fwd[i]);
            }
            // the block subtrees, leaves first
            const uint32_t* child = nullptr;
            for (uint32_t l = Lmax; l + 1 > b; l--) {
                rsv::CmHashArgs a = cm_layer_args(g, ng, b, l, at, Pc, nb);
                a.child = child;
                a.blk0 = (uint32_t)blk0;
                a.out = l == b ? w.broots : ((Lmax - l) & 1 ? w.nbuf : w.na);
                hipLaunchKernelGGL(rsv::k_cm_hash_layer, dim3(grid_for((size_t)Pc * nb << a.lw, 256)), dim3(256), 0, st, a);
                child = a.out;
            }
        }
        // the plain node layers above the block roots; each level also goes to the cap where one is asked for
        auto to_cap = [&](const uint32_t* lvl, uint64_t stride, uint32_t l) {
            if (d_cap)
                hipLaunchKernelGGL(rsv::k_cm_cap_level, dim3(grid_for(Pc << l, 256)), dim3(256), 0, st, lvl, stride, d_cap, cap_stride, l,
                                   (uint32_t)Pc, d_mask, (uint32_t)p0);
        };
        const uint32_t* in = w.broots;
        to_cap(w.broots, (uint64_t)8 << b, b);
        for (uint32_t l = b; l-- > 0;) {
            uint32_t* out = (b - 1 - l) & 1 ? w.tb : w.ta;
            hipLaunchKernelGGL(rsv::k_cm_top, dim3(grid_for(Pc << l, 256)), dim3(256), 0, st, in, out, l, (uint32_t)Pc, d_roots, roots_stride,
                               d_mask, (uint32_t)p0);
            if (l) to_cap(out, (uint64_t)8 << l, l);
            else to_cap(d_roots + p0 * roots_stride, roots_stride, 0);
            in = out;
        }
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

// Any of the pointers null; any of them off a 4-byte boundary (a null pointer is aligned).
template <class... P>
bool any_null(const P*... p) {
    return (... || !p);
}
template <class... P>
bool any_misaligned(const P*... p) {
    return (... || ((uintptr_t)p & 3));
}

// What every stage of the chain takes first: the context, the program, the proofs' trace and interaction columns (d_ops may
// be null), the flags and the batch.  A stage tests chain_null and chain_misaligned with its own pointers added, then its
// own sizes, then calls chain_open.  The two tests are not inside chain_open because a null pointer of any kind, shared or
// the stage's own, is RSV_E_NULL before any misalignment or size is RSV_E_SIZE, and each stage's size checks stand between
// the tests and chain_open's body: one call could only keep that order by taking the stage's pointers and sizes as well.
struct ChainArgs {
    rsv_ctx* c;
    const rsv_witness_program* prog;
    const uint32_t *plonk, *poseidon, *ops, *int_plonk, *int_poseidon;
    const uint8_t *accept, *ok;
    size_t n;
    uint32_t log_blowup;
};
template <class... P>
bool chain_null(const ChainArgs& a, const P*... stage) {
    return any_null(a.c, a.prog, a.plonk, a.poseidon, a.int_plonk, a.int_poseidon, a.accept, stage...);
}
template <class... P>
bool chain_misaligned(const ChainArgs& a, const P*... stage) {
    return any_misaligned(a.plonk, a.poseidon, a.ops, a.int_plonk, a.int_poseidon, stage...);
}

// The three trees of the recursion circuit's next proof as commit groups, the mask of the stages behind the commitment
// (d_ok where given, else d_accept), and the chain's workspace: tree 0's op column of every proof (column 3 of the Plonk
// preprocessed ones follows the proof, the other 49 are the program's), the lookup elements, the channels and the ok flags
// between the trees.
struct ChainTrees {
    rsv_commit_group t0[4], t1[2], t2[2];
    const uint8_t* mask;
    uint32_t *lookup, *chan;
    uint8_t* ok;
    const rsv_commit_group* tree(int t) const { return t == 0 ? t0 : t == 1 ? t1 : t2; }
};
constexpr size_t CHAIN_TREE_GROUPS[3] = {4, 2, 2};

// sampled_values[0..2] of the next proof, group by group in the proof's own order: the tree, the group within it
// (ChainTrees) and which of its columns (the interaction groups are cut into columns 0..3, one value each, and the
// cumulative 4..7, two each: the previous-row value, then the OODS value); the entry of the first column's OODS value, the
// step from column to column, and which previous-row point the group has (0: none, 1: the Plonk step, 2: the Poseidon one).
// A cut group has two rows, the cumulative half straight after the other: rsv_witness_sample_dev samples the group whole
// from the first row, and its output form (SpOut, chain == 1, single == the first row's cols, two points) puts the
// cumulative columns' OODS values at entry + cols + 1, step 2.  chain_samples_before holds the second row to that.
struct ChainSamples {
    uint32_t tree, group, col0, cols, entry, step, prev_point;
};
constexpr ChainSamples CHAIN_SAMPLES[10] = {
    {0, 0, 0, 3, 0, 1, 0},   {0, 1, 0, 1, 3, 1, 0},   {0, 2, 0, 6, 4, 1, 0},   {0, 3, 0, 40, 10, 1, 0},  {1, 0, 0, 12, 50, 1, 0},
    {1, 1, 0, 48, 62, 1, 0}, {2, 0, 0, 4, 110, 1, 0}, {2, 0, 4, 4, 115, 2, 1}, {2, 1, 0, 4, 122, 1, 0}, {2, 1, 4, 4, 127, 2, 2}};
// The values of the table's first k groups; 0 unless each group starts where the one before ends, only a cumulative half
// has a previous-row point and the step of 2 that goes with it, and such a half follows the first half of its own group.
constexpr uint32_t chain_samples_before(size_t k) {
    uint32_t at = 0;
    for (size_t i = 0; i < k; i++) {
        const ChainSamples& s = CHAIN_SAMPLES[i];
        if (s.entry != at + (s.prev_point ? 1 : 0) || s.step != (s.prev_point ? 2u : 1u) || (s.col0 != 0) != (s.prev_point != 0)) return 0;
        if (s.col0) {
            if (i == 0) return 0;
            const ChainSamples& h = CHAIN_SAMPLES[i - 1];
            if (h.tree != s.tree || h.group != s.group || h.col0 != 0 || h.cols != s.col0) return 0;
        }
        at += s.cols * s.step;
    }
    return at;
}
constexpr uint32_t CHAIN_SAMPLE_VALUES = chain_samples_before(10);
static_assert(CHAIN_SAMPLE_VALUES == 134, "trees 0, 1 and 2: 50 + 60 + 24 sampled values");

// Enqueues the op column on the context's stream.
int chain_open(const ChainArgs& a, ChainTrees* ct) {
    rsv_ctx* c = a.c;
    const rsv_witness_program* prog = a.prog;
    const uint32_t *d_plonk = a.plonk, *d_poseidon = a.poseidon, *d_ops = a.ops, *d_int_plonk = a.int_plonk, *d_int_poseidon = a.int_poseidon;
    const size_t n = a.n;
    const uint32_t log_blowup = a.log_blowup;
    ct->mask = a.ok ? a.ok : a.accept;
    int rc = chain_begin(c, prog, n, true);
    if (rc != RSV_OK) return rc;
    const uint32_t lp = prog->trace_lp, lq = prog->trace_lq;
    if (std::max(lp, lq) + log_blowup > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;
    const size_t n_ops = prog->witness_ops.size() / 3;
    if (n_ops && !d_ops) return RSV_E_NULL;
    if (n == 0) return RSV_OK;
    const size_t N = (size_t)1 << lp, Q = (size_t)1 << lq;
    if (((uint64_t)n * N) / 256 >= (1u << 31)) return RSV_E_SIZE;
    rsv::host::Carve sz{nullptr};
    sz.take<uint32_t>(n * N);
    sz.take<uint32_t>(n * 8);
    sz.take<uint32_t>(n * 16);
    sz.take<uint8_t>(n);
    rc = ensure_buf(c, &c->ws_chain, &c->ws_chain_bytes, sz.off);
    if (rc != RSV_OK) return rc;
    rsv::host::Carve cv{static_cast<char*>(c->ws_chain)};
    uint32_t* ops_col = cv.take<uint32_t>(n * N);
    ct->lookup = cv.take<uint32_t>(n * 8);
    ct->chan = cv.take<uint32_t>(n * 16);
    ct->ok = cv.take<uint8_t>(n);
    hipStream_t st = c->stream;
    const uint32_t* pre = prog->d_trace_pre;
    const uint32_t* qpre = pre + rsv::trace::PLONK_PRE_COLS * N;
    hipLaunchKernelGGL(rsv::k_cm_op_column, dim3(grid_for(n * N, 256)), dim3(256), 0, st, pre + 3 * N, lp, (uint32_t)n, ops_col);
    if (n_ops)
        hipLaunchKernelGGL(rsv::k_cm_op_patch, dim3(grid_for(n_ops * n, 256)), dim3(256), 0, st, prog->d_trace_ops, (uint32_t)n_ops, d_ops, lp,
                           (uint32_t)n, ops_col);
    ct->t0[0] = {lp, 3, pre, 0, nullptr, nullptr};
    ct->t0[1] = {lp, 1, ops_col, N, nullptr, nullptr};
    ct->t0[2] = {lp, 6, pre + 4 * N, 0, nullptr, nullptr};
    ct->t0[3] = {lq, rsv::trace::POSEIDON_PRE_COLS, qpre, 0, nullptr, nullptr};
    ct->t1[0] = {lp, rsv::PLONK_COLS_K, d_plonk, rsv::PLONK_COLS_K * N, nullptr, nullptr};  // the 12 + 48 trace columns
    ct->t1[1] = {lq, rsv::POSEIDON_COLS_K, d_poseidon, rsv::POSEIDON_COLS_K * Q, nullptr, nullptr};
    ct->t2[0] = {lp, rsv::INT_COLS, d_int_plonk, rsv::INT_COLS * N, nullptr, nullptr};
    ct->t2[1] = {lq, rsv::INT_COLS, d_int_poseidon, rsv::INT_COLS * Q, nullptr, nullptr};
    return RSV_OK;
}

}  // namespace

extern "C" {

int rsv_commit_tree_dev(rsv_ctx* c, const rsv_commit_group* groups, size_t n_groups, size_t n, uint32_t log_blowup, const uint8_t* d_mask,
                        uint32_t* d_roots) {
    return commit_tree(c, groups, n_groups, n, log_blowup, d_mask, d_roots, 8);
}

int rsv_commit_tree_cap_dev(rsv_ctx* c, const rsv_commit_group* groups, size_t n_groups, size_t n, uint32_t log_blowup,
                            const uint8_t* d_mask, uint32_t* d_roots, uint32_t* d_cap) {
    return commit_tree(c, groups, n_groups, n, log_blowup, d_mask, d_roots, 8, d_cap, (uint64_t)16 << log_blowup);
}

int rsv_witness_commit_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                           const uint32_t* d_ops, const uint8_t* d_accept, size_t n, uint32_t log_blowup, uint32_t* d_roots,
                           uint32_t* d_draws, uint32_t* d_int_plonk, uint32_t* d_int_poseidon, uint32_t* d_sums, uint32_t* d_channel,
                           uint8_t* d_ok) {
    return rsv_witness_commit_caps_dev(c, prog, d_plonk, d_poseidon, d_ops, d_accept, n, log_blowup, d_roots, d_draws, d_int_plonk,
                                       d_int_poseidon, d_sums, d_channel, d_ok, nullptr);
}

int rsv_witness_commit_caps_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                                const uint32_t* d_ops, const uint8_t* d_accept, size_t n, uint32_t log_blowup, uint32_t* d_roots,
                                uint32_t* d_draws, uint32_t* d_int_plonk, uint32_t* d_int_poseidon, uint32_t* d_sums, uint32_t* d_channel,
                                uint8_t* d_ok, uint32_t* d_caps) {
    // the commitment's own mask is d_accept (d_ok is its output)
    const ChainArgs a{c, prog, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, nullptr, n, log_blowup};
    if (chain_null(a, d_roots, d_draws, d_sums)) return RSV_E_NULL;
    if (log_blowup < 1 || log_blowup > RSV_MAX_LOG_BLOWUP) return RSV_E_SIZE;
    if (chain_misaligned(a, d_roots, d_draws, d_sums, d_channel, d_caps) || ((uintptr_t)d_int_plonk & 7) || ((uintptr_t)d_int_poseidon & 7))
        return RSV_E_SIZE;
    ChainTrees ct;
    int rc = chain_open(a, &ct);
    if (rc != RSV_OK || n == 0) return rc;
    const uint32_t lp = prog->trace_lp, lq = prog->trace_lq;
    hipStream_t st = c->stream;
    const uint64_t cap1 = (uint64_t)16 << log_blowup, cap3 = 3 * cap1;  // words of one tree's cap, of a proof's three
    rc = commit_tree(c, ct.t0, 4, n, log_blowup, d_accept, d_roots, 24, d_caps, cap3);
    if (rc != RSV_OK) return rc;
    rc = commit_tree(c, ct.t1, 2, n, log_blowup, d_accept, d_roots + 8, 24, d_caps ? d_caps + cap1 : nullptr, cap3);
    if (rc != RSV_OK) return rc;
    hipLaunchKernelGGL(rsv::k_cm_draw_lookup, dim3(grid_for(n, 64)), dim3(64), 0, st, d_roots, lp, lq, (uint32_t)n, ct.lookup, ct.chan);
    // tree 2: the interaction columns under the drawn (z, alpha)
    rc = rsv_witness_interaction_dev(c, prog, d_plonk, d_poseidon, d_accept, ct.lookup, n, d_int_plonk, d_int_poseidon, d_sums, ct.ok);
    if (rc != RSV_OK) return rc;
    rc = commit_tree(c, ct.t2, 2, n, log_blowup, ct.ok, d_roots + 16, 24, d_caps ? d_caps + 2 * cap1 : nullptr, cap3);
    if (rc != RSV_OK) return rc;
    hipLaunchKernelGGL(rsv::k_cm_draw_coeff, dim3(grid_for(n, 64)), dim3(64), 0, st, d_roots, ct.lookup, d_sums, ct.ok, (uint32_t)n, ct.chan,
                       d_draws, d_channel, d_ok);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int rsv_witness_commit(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                       const rsv_public_input* pi, size_t n_pi, uint32_t log_blowup, uint32_t* roots, uint32_t* draws, uint32_t* sums,
                       uint8_t* ok, uint8_t* accept, uint8_t* reason, int device) {
    return nomem_guard([&]() -> int {
        if (!prog || (n && (!blob || !offsets || !roots || !draws || !sums || !accept))) return RSV_E_NULL;
        if (log_blowup < 1 || log_blowup > RSV_MAX_LOG_BLOWUP) return RSV_E_SIZE;
        if (prog->gates.empty() || prog->n_instr == 0 || n > (1u << 20)) return RSV_E_SIZE;  // built programs only: the witness is evaluated
        if (n == 0) return RSV_OK;
        WitnessStage st;
        int rc = st.open(offsets, n, device, true);
        if (rc == RSV_OK) rc = program_upload(const_cast<rsv_witness_program*>(prog), true);
        if (rc != RSV_OK) return rc;
        if (std::max(prog->trace_lp, prog->trace_lq) + log_blowup > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;
        const size_t N = (size_t)1 << prog->trace_lp, Q = (size_t)1 << prog->trace_lq;
        const size_t n_ops = prog->witness_ops.size() / 3;
        HostStage& s = st.b.s;
        uint32_t* dplonk = s.scratch<uint32_t>(n * rsv::PLONK_COLS_K * N * 4);
        uint32_t* dposeidon = s.scratch<uint32_t>(n * rsv::POSEIDON_COLS_K * Q * 4);
        uint32_t* dops = s.scratch<uint32_t>(n * n_ops * 4);
        uint32_t* dip = s.scratch<uint32_t>(n * rsv::INT_COLS * N * 4);
        uint32_t* diq = s.scratch<uint32_t>(n * rsv::INT_COLS * Q * 4);
        uint32_t* droots = s.output<uint32_t>(roots, n * 96);
        uint32_t* ddraws = s.output<uint32_t>(draws, n * 48);
        uint32_t* dsums = s.output<uint32_t>(sums, n * 32);
        uint8_t* dok = ok ? s.output<uint8_t>(ok, n) : s.scratch<uint8_t>(n);
        if (s.rc != RSV_OK) return s.rc;
        rc = st.eval(prog, blob, cfg, pi, n_pi, true);
        if (rc == RSV_OK) rc = rsv_witness_trace_dev(st.c(), prog, st.vars, st.flow, st.swap, st.accept, n, dplonk, dposeidon, dops);
        if (rc == RSV_OK)
            rc = rsv_witness_commit_dev(st.c(), prog, dplonk, dposeidon, dops, st.accept, n, log_blowup, droots, ddraws, dip, diq, dsums, nullptr, dok);
        return rc == RSV_OK ? st.finish(accept, reason) : rc;
    });
}

}  // extern "C"
