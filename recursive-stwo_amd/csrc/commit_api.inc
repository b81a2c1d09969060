// commit_api.inc — rsv_commit_tree_dev / rsv_commit_tree_cap_dev (a generic tree commitment: interpolation, LDE, mixed-size
// Merkle tree, optionally leaving the tree's cap) and rsv_witness_commit_dev / rsv_witness_commit_caps_dev /
// rsv_witness_commit (trees 0, 1, 2 of the recursion circuit's next proof and the transcript draws between them):
// k_commit.hpp, include/rsv.h.  Included at the end of rsv_hip.hip, after interaction_api.inc; decommit_api.inc follows.

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

// Workspace of a pass of P proofs and nb blocks (bytes, with Carve's alignment); with cv, also where each part goes.
size_t cm_ws_bytes(const rsv_commit_group* g, size_t ng, uint32_t b, uint32_t Lmax, size_t P, size_t nb, rsv::host::Carve* cv,
                   uint32_t** coef, uint32_t** lde, uint32_t** nodes_a, uint32_t** nodes_b, uint32_t** broots, uint32_t** top_a,
                   uint32_t** top_b) {
    rsv::host::Carve sz{cv ? cv->base : nullptr};
    for (size_t i = 0; i < ng; i++) {
        const size_t row = (size_t)1 << g[i].log_size;
        uint32_t* p = g[i].d_coeffs ? nullptr : sz.take<uint32_t>(P * g[i].n_cols * row);
        if (coef) coef[i] = p;
        uint32_t* q = g[i].d_lde ? nullptr : sz.take<uint32_t>(P * g[i].n_cols * nb * row);
        if (lde) lde[i] = q;
    }
    const size_t leaves = P * nb << (Lmax - b);
    uint32_t* a = sz.take<uint32_t>(leaves * 8);
    uint32_t* bb = sz.take<uint32_t>(std::max<size_t>(leaves / 2, 1) * 8);
    uint32_t* r = sz.take<uint32_t>((P << b) * 8);
    uint32_t* ta = sz.take<uint32_t>((P << (b - 1)) * 8);
    uint32_t* tb = sz.take<uint32_t>((P << (b - 1)) * 8);
    if (nodes_a) { *nodes_a = a; *nodes_b = bb; *broots = r; *top_a = ta; *top_b = tb; }
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
    // the largest pass within the budget: all blocks of all proofs, then fewer blocks, then fewer proofs
    const size_t budget = ws_budget(c);
    size_t P = n, nb = (size_t)1 << b;
    while (cm_ws_bytes(g, ng, b, Lmax, P, nb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) > budget && nb > 1) nb >>= 1;
    while (cm_ws_bytes(g, ng, b, Lmax, P, nb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) > budget && P > 1) P = (P + 1) / 2;
    // every launch's grid stays below 2^31 workgroups
    const uint64_t lim = (uint64_t)1 << 31;
    for (size_t i = 0; i < ng; i++) {
        const uint64_t n_rows = (uint64_t)P * g[i].n_cols * nb;
        if (n_rows >= lim || (n_rows << g[i].log_size) / 256 >= lim || ((uint64_t)P * g[i].n_cols << g[i].log_size) / 256 >= lim) return RSV_E_SIZE;
    }
    if (((uint64_t)P * nb << (Lmax - b)) / 256 >= lim) return RSV_E_SIZE;
    const uint32_t* tw_inv[RSV_MAX_COMMIT_GROUPS];
    const uint32_t* tw_fwd[RSV_MAX_COMMIT_GROUPS];
    for (size_t i = 0; i < ng; i++) {
        int rc = cm_twiddles(c, g[i].log_size, true, &tw_inv[i]);
        if (rc == RSV_OK) rc = cm_twiddles(c, g[i].log_size + b, false, &tw_fwd[i]);
        if (rc != RSV_OK) return rc;
    }
    const size_t need = cm_ws_bytes(g, ng, b, Lmax, P, nb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    int rc = ensure_buf(c, &c->ws_commit, &c->ws_commit_bytes, need);
    if (rc != RSV_OK) return rc;
    rsv::host::Carve cv{static_cast<char*>(c->ws_commit)};
    uint32_t *coef[RSV_MAX_COMMIT_GROUPS], *lde[RSV_MAX_COMMIT_GROUPS], *na, *nbuf, *broots, *ta, *tb;
    cm_ws_bytes(g, ng, b, Lmax, P, nb, &cv, coef, lde, &na, &nbuf, &broots, &ta, &tb);
    hipStream_t st = c->stream;
    for (size_t p0 = 0; p0 < n; p0 += P) {
        const size_t Pc = std::min(P, n - p0);
        // interpolation: the columns -> the coefficients (d_coeffs or the workspace), masked proofs zero
        uint32_t* cf[RSV_MAX_COMMIT_GROUPS];
        for (size_t i = 0; i < ng; i++) {
            const uint32_t log = g[i].log_size, cols = g[i].n_cols;
            const size_t row = (size_t)1 << log;
            cf[i] = g[i].d_coeffs ? g[i].d_coeffs + p0 * cols * row : coef[i];
            rsv::CmRows r{cf[i], row, (uint64_t)Pc * cols, log, log, 1, 0};
            rsv::CmSrc s{g[i].d_cols + p0 * g[i].proof_stride, g[i].proof_stride, row, d_mask, cols, (uint32_t)p0,
                         log ? 1u << (31 - log) : 1u};  // 2^-log = 2^(31-log) mod P
            cm_fft<true>(st, r, s, tw_inv[i]);
        }
        for (size_t blk0 = 0; blk0 < ((size_t)1 << b); blk0 += nb) {
            // the LDE of blocks blk0 .. blk0 + nb - 1
            for (size_t i = 0; i < ng; i++) {
                const uint32_t log = g[i].log_size, cols = g[i].n_cols, N = log + b;
                const size_t row = (size_t)1 << log;
                rsv::CmRows r{};
                if (g[i].d_lde) r = {g[i].d_lde + p0 * cols * ((size_t)1 << N) + (blk0 << log), (uint64_t)1 << N, 0, log, N, (uint32_t)nb, (uint32_t)blk0};
                else r = {lde[i], (uint64_t)nb << log, 0, log, N, (uint32_t)nb, (uint32_t)blk0};
                r.rows = (uint64_t)Pc * cols * nb;
                rsv::CmSrc s{cf[i], (uint64_t)cols * row, row, nullptr, cols, 0, 1};
                cm_fft<false>(st, r, s, tw_fwd[i]);
            }
            // the block subtrees, leaves first
            const uint32_t* child = nullptr;
            for (uint32_t l = Lmax; l + 1 > b; l--) {
                rsv::CmHashArgs a{};
                a.lw = l - b;
                a.nb = (uint32_t)nb;
                a.P = (uint32_t)Pc;
                a.child = child;
                a.b = b;
                a.blk0 = (uint32_t)blk0;
                for (size_t i = 0; i < ng; i++) {
                    if (g[i].log_size + b != l) continue;
                    rsv::CmLayerCols& lc = a.g[a.ng++];
                    lc.n_cols = g[i].n_cols;
                    if (g[i].d_lde) {
                        lc.base = g[i].d_lde + p0 * g[i].n_cols * ((size_t)1 << l) + (blk0 << g[i].log_size);
                        lc.pc_stride = (uint64_t)1 << l;
                    } else {
                        lc.base = lde[i];
                        lc.pc_stride = (uint64_t)nb << g[i].log_size;
                    }
                    a.n_cols += g[i].n_cols;
                }
                a.out = l == b ? broots : ((Lmax - l) & 1 ? nbuf : na);
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
        const uint32_t* in = broots;
        to_cap(broots, (uint64_t)8 << b, b);
        for (uint32_t l = b; l-- > 0;) {
            uint32_t* out = (b - 1 - l) & 1 ? tb : ta;
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
    if (!prog || (n && (!blob || !offsets || !roots || !draws || !sums || !accept))) return RSV_E_NULL;
    if (log_blowup < 1 || log_blowup > RSV_MAX_LOG_BLOWUP) return RSV_E_SIZE;
    if (prog->gates.empty() || n > (1u << 20)) return RSV_E_SIZE;  // built programs only, as rsv_witness_commit_dev
    if (n == 0) return RSV_OK;
    WitnessStage st;
    int rc = st.open(offsets, n, device, true);
    if (rc == RSV_OK) rc = program_upload(const_cast<rsv_witness_program*>(prog), true);
    if (rc != RSV_OK) return rc;
    if (std::max(prog->trace_lp, prog->trace_lq) + log_blowup > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;
    const size_t N = (size_t)1 << prog->trace_lp, Q = (size_t)1 << prog->trace_lq;
    const size_t n_ops = prog->witness_ops.size() / 3;
    DevBuf dplonk, dposeidon, dops, dip, diq, droots, ddraws, dsums, dok;
    HIP_TRY(dplonk.alloc(n * rsv::PLONK_COLS_K * N * 4));
    HIP_TRY(dposeidon.alloc(n * rsv::POSEIDON_COLS_K * Q * 4));
    HIP_TRY(dops.alloc(n * n_ops * 4));
    HIP_TRY(dip.alloc(n * rsv::INT_COLS * N * 4));
    HIP_TRY(diq.alloc(n * rsv::INT_COLS * Q * 4));
    HIP_TRY(droots.alloc(n * 96));
    HIP_TRY(ddraws.alloc(n * 48));
    HIP_TRY(dsums.alloc(n * 32));
    HIP_TRY(dok.alloc(n));
    rc = st.eval(prog, blob, cfg, pi, n_pi, true);
    if (rc == RSV_OK)
        rc = rsv_witness_trace_dev(st.c, prog, st.vars, st.flow, st.swap, st.accept, n, dplonk.as<uint32_t>(), dposeidon.as<uint32_t>(),
                                   dops.as<uint32_t>());
    if (rc == RSV_OK)
        rc = rsv_witness_commit_dev(st.c, prog, dplonk.as<const uint32_t>(), dposeidon.as<const uint32_t>(), dops.as<const uint32_t>(),
                                    st.accept, n, log_blowup, droots.as<uint32_t>(), ddraws.as<uint32_t>(), dip.as<uint32_t>(),
                                    diq.as<uint32_t>(), dsums.as<uint32_t>(), nullptr, dok.as<uint8_t>());
    if (rc == RSV_OK) rc = st.finish(accept, reason);
    if (rc != RSV_OK) return rc;
    HIP_TRY(hipMemcpy(roots, droots.p, n * 96, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(draws, ddraws.p, n * 48, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sums, dsums.p, n * 32, hipMemcpyDeviceToHost));
    if (ok) HIP_TRY(hipMemcpy(ok, dok.p, n, hipMemcpyDeviceToHost));
    return RSV_OK;
}

}  // extern "C"
