// decommit_api.inc — rsv_decommit_sizes, rsv_decommit_tree_dev (the opening of a streamed tree at a list of positions:
// queried values and Merkle witness in stwo's batched order) and rsv_witness_decommit_dev (trees 0, 1, 2 of the recursion
// circuit's next proof): k_decommit.hpp, include/rsv.h.  Included at the end of rsv_hip.hip, after commit_api.inc.
//
// decommit_tree streams the groups with commit_api.inc's helpers; its blocks are entries of the proofs' block lists, so
// it takes the extension as a pair (cm_extension) and launches it on the block-list kernels (dc_fft, k_dc_hash_layer).

namespace {

struct DcWs {
    uint32_t *coef[RSV_MAX_COMMIT_GROUPS], *lde[RSV_MAX_COMMIT_GROUPS], *na, *nbuf, *cap;
    rsv::DcPlan pl;
};

// Workspace of an opening: the plan of all n proofs, and of a pass of P proofs and nb list entries (blocks) the
// coefficients, the blocks in flight, two node layers and (own_cap) the caps.  With w, also where each part goes.
size_t dc_ws_bytes(const rsv_commit_group* g, size_t ng, uint32_t b, uint32_t top, size_t n, uint32_t nq, size_t maxb, size_t P, size_t nb,
                   bool own_cap, char* base, DcWs* w) {
    rsv::host::Carve sz{base};
    DcWs t{};
    const size_t wcap = (size_t)nq * top;
    t.pl.cnt = sz.take<uint32_t>(n);
    t.pl.blocks = sz.take<uint32_t>(n * maxb);
    t.pl.nl = sz.take<uint32_t>(n * rsv::DC_LAYERS);
    t.pl.voff = sz.take<uint32_t>(n * rsv::DC_LAYERS);
    t.pl.woff = sz.take<uint32_t>(n * rsv::DC_LAYERS);
    t.pl.node = sz.take<uint32_t>(n * (top + 1) * nq);
    t.pl.nodek = sz.take<uint32_t>(n * (top + 1) * nq);
    t.pl.wnode = sz.take<uint32_t>(n * wcap);
    t.pl.wk = sz.take<uint32_t>(n * wcap);
    t.pl.maxb = (uint32_t)maxb;
    t.pl.nq = nq;
    t.pl.wcap = (uint32_t)wcap;
    t.pl.top = top;
    t.pl.b = b;
    for (size_t i = 0; i < ng; i++) {
        const size_t row = (size_t)1 << g[i].log_size;
        t.coef[i] = sz.take<uint32_t>(P * g[i].n_cols * row);
        t.lde[i] = sz.take<uint32_t>(P * g[i].n_cols * nb * row);
    }
    const size_t leaves = P * nb << (top - b);
    t.na = sz.take<uint32_t>(leaves * 8);
    t.nbuf = sz.take<uint32_t>(std::max<size_t>(leaves / 2, 1) * 8);
    t.cap = own_cap ? sz.take<uint32_t>((P << (b + 1)) * 8) : nullptr;
    if (w) *w = t;
    return sz.off;
}

// The plan's view from proof p0 on.
rsv::DcPlan dc_plan_at(rsv::DcPlan pl, size_t p0) {
    pl.cnt += p0;
    pl.blocks += p0 * pl.maxb;
    pl.nl += p0 * rsv::DC_LAYERS;
    pl.voff += p0 * rsv::DC_LAYERS;
    pl.woff += p0 * rsv::DC_LAYERS;
    pl.node += p0 * (pl.top + 1) * pl.nq;
    pl.nodek += p0 * (pl.top + 1) * pl.nq;
    pl.wnode += p0 * pl.wcap;
    pl.wk += p0 * pl.wcap;
    return pl;
}

// The forward FFT of the listed blocks (cm_fft<false> with the block-list kernels).
void dc_fft(hipStream_t st, const rsv::CmRows& r, const rsv::CmSrc& s, const uint32_t* tw, const rsv::CmList& L) {
    const uint32_t c = std::min(r.log, rsv::CM_LDS_LOG);
    const rsv::CmSrc none{};
    const uint64_t pairs = r.rows << (r.log ? r.log - 1 : 0);
    for (uint32_t m = r.log; m-- > c;)
        hipLaunchKernelGGL(rsv::k_dc_fft_layer, dim3(grid_for(pairs, 256)), dim3(256), 0, st, r, m + 1 == r.log ? s : none, tw, m, L);
    hipLaunchKernelGGL(rsv::k_dc_fft_lds, dim3((unsigned)(r.rows << (r.log - c))), dim3(256), 0, st, r, r.log > c ? none : s, tw, c, L);
}

void decommit_caps(const rsv_commit_group* g, size_t ng, uint32_t b, uint32_t nq, uint32_t* top, size_t* values_cap, size_t* witness_cap) {
    uint32_t t = 0;
    size_t cols = 0;
    for (size_t i = 0; i < ng; i++) {
        t = std::max(t, g[i].log_size + b);
        cols += g[i].n_cols;
    }
    *top = t;
    *values_cap = (size_t)nq * cols;
    *witness_cap = (size_t)nq * t;
}

// Outputs of proof i at d_values + i * vstride (words; values_cap of them written), d_witness + i * wstride (witness_cap
// nodes), d_n_values + i * nstride, d_n_witness + i * nstride, d_cap + i * cap_stride.
int decommit_tree(rsv_ctx* c, const rsv_commit_group* g, size_t ng, size_t n, uint32_t b, const uint8_t* d_mask, const uint32_t* d_queries,
                  uint32_t nq, int mode, uint32_t* d_cap, uint64_t cap_stride, uint32_t* d_values, uint64_t vstride, uint32_t* d_n_values,
                  uint32_t* d_witness, uint64_t wstride, uint32_t* d_n_witness, uint32_t nstride) {
    if (!c || !g || !d_queries || !d_values || !d_n_values || !d_witness || !d_n_witness) return RSV_E_NULL;
    if (mode != RSV_CAP_NONE && mode != RSV_CAP_WRITE && mode != RSV_CAP_READ) return RSV_E_SIZE;
    if (mode != RSV_CAP_NONE && !d_cap) return RSV_E_NULL;
    if (ng == 0 || ng > RSV_MAX_COMMIT_GROUPS || n > (1u << 20) || b < 1 || b > RSV_MAX_LOG_BLOWUP || nq < 1 || nq > RSV_MAX_QUERIES)
        return RSV_E_SIZE;
    if (((uintptr_t)d_queries & 3) || ((uintptr_t)d_values & 3) || ((uintptr_t)d_n_values & 3) || ((uintptr_t)d_witness & 3) ||
        ((uintptr_t)d_n_witness & 3) || ((uintptr_t)d_cap & 3))
        return RSV_E_SIZE;
    for (size_t i = 0; i < ng; i++) {
        if (!g[i].d_cols) return RSV_E_NULL;
        if (g[i].n_cols == 0 || g[i].n_cols > 0xffff || g[i].log_size + b > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;
        if ((uintptr_t)g[i].d_cols & 3) return RSV_E_SIZE;
    }
    uint32_t top;
    size_t vcap, wcap;
    decommit_caps(g, ng, b, nq, &top, &vcap, &wcap);
    rsv::DcCols nc{};
    for (size_t i = 0; i < ng; i++) {
        const uint32_t l = g[i].log_size + b;
        if ((uint32_t)nc.n[l] + g[i].n_cols > 0xffff) return RSV_E_SIZE;
        nc.n[l] = (uint16_t)(nc.n[l] + g[i].n_cols);
    }
    if (n == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    const bool full = mode != RSV_CAP_READ, own_cap = mode == RSV_CAP_NONE;
    // a pass is P proofs times nb entries of their block lists
    const size_t maxb = full ? (size_t)1 << b : std::min<size_t>(nq, (size_t)1 << b);
    const auto ws = [&](size_t P, size_t nb, char* base = nullptr, DcWs* w = nullptr) {
        return dc_ws_bytes(g, ng, b, top, n, nq, maxb, P, nb, own_cap, base, w);
    };
    const rsv::host::Pass pass = rsv::host::plan_pass(ws_budget(c), n, maxb, ws);
    const size_t P = pass.P, nb = pass.nb;
    for (size_t i = 0; i < ng; i++)
        if (!cm_rows_fit((uint64_t)P * g[i].n_cols * nb, g[i].log_size)) return RSV_E_SIZE;
    if (((uint64_t)P * nb << (top - b)) / 256 >= CM_GRID_LIM || ((uint64_t)n * std::max(vcap, wcap * 8)) / 256 >= CM_GRID_LIM ||
        (full && ((uint64_t)n << (b + 4)) / 256 >= CM_GRID_LIM))
        return RSV_E_SIZE;
    const uint32_t *tw_inv[RSV_MAX_COMMIT_GROUPS], *tw_fwd[RSV_MAX_COMMIT_GROUPS];
    int rc = cm_group_twiddles(c, g, ng, b, tw_inv, tw_fwd);
    DcWs w;
    if (rc == RSV_OK) rc = cm_workspace(c, [&](char* base) { return ws(P, nb, base, &w); });
    if (rc != RSV_OK) return rc;
    hipStream_t st = c->stream;
    // every element of the outputs is defined: zero, then the planned words
    hipLaunchKernelGGL(rsv::k_dc_zero, dim3(grid_for(n * vcap, 256)), dim3(256), 0, st, d_values, vstride, (uint64_t)vcap, (uint64_t)n);
    hipLaunchKernelGGL(rsv::k_dc_zero, dim3(grid_for(n * wcap * 8, 256)), dim3(256), 0, st, d_witness, wstride, (uint64_t)wcap * 8, (uint64_t)n);
    if (mode == RSV_CAP_WRITE)  // a masked proof's cap
        hipLaunchKernelGGL(rsv::k_dc_zero, dim3(grid_for(n << (b + 4), 256)), dim3(256), 0, st, d_cap, cap_stride, (uint64_t)16 << b, (uint64_t)n);
    hipLaunchKernelGGL(rsv::k_dc_plan, dim3((unsigned)n), dim3(128), 0, st, d_queries, d_mask, nc, w.pl, full ? 1u : 0u, d_n_values, nstride,
                       d_n_witness, nstride);
    const uint64_t cstride = own_cap ? (uint64_t)16 << b : cap_stride;
    for (size_t p0 = 0; p0 < n; p0 += P) {
        const size_t Pc = std::min(P, n - p0);
        const rsv::DcPlan pl = dc_plan_at(w.pl, p0);
        const rsv::DcOut out{d_values + p0 * vstride, d_witness + p0 * wstride, vstride, wstride};
        uint32_t* cap = own_cap ? w.cap : d_cap + p0 * cap_stride;
        for (size_t i = 0; i < ng; i++) cm_interpolate(st, g[i], w.coef[i], p0, Pc, d_mask, false, tw_inv[i]);
        for (size_t k0 = 0; k0 < maxb; k0 += nb) {
            const size_t nbc = std::min(nb, maxb - k0);
            rsv::CmList L{pl.blocks, pl.cnt, (uint32_t)maxb, (uint32_t)k0, 0, cstride};
            // the LDE of the list's entries k0 .. k0 + nbc - 1
            CmBlocks at[RSV_MAX_COMMIT_GROUPS];
            for (size_t i = 0; i < ng; i++) {
                const uint32_t log = g[i].log_size, cols = g[i].n_cols;
                at[i] = {w.lde[i], (uint64_t)nbc << log};
                L.cols = cols;
                const CmExt e = cm_extension(g[i], w.coef[i], (uint64_t)cols << log, (uint64_t)Pc * cols, log + b, nbc, 0, at[i]);
                dc_fft(st, e.r, e.s, tw_fwd[i], L);
            }
            // their subtrees, leaves first; after each layer, what the plan takes from it
            const uint32_t* child = nullptr;
            for (uint32_t l = top; l + 1 > b; l--) {
                rsv::CmHashArgs a = cm_layer_args(g, ng, b, l, at, Pc, nbc);
                a.child = child;
                a.out = l == b ? cap : ((top - l) & 1 ? w.nbuf : w.na);
                if (l > b || full)
                    hipLaunchKernelGGL(rsv::k_dc_hash_layer, dim3(grid_for((size_t)Pc * nbc << a.lw, 256)), dim3(256), 0, st, a, L);
                if (l > b || a.n_cols)
                    hipLaunchKernelGGL(rsv::k_dc_gather, dim3(grid_for((size_t)Pc * nq * (8 + a.n_cols), 256)), dim3(256), 0, st, a, pl, out,
                                       (uint32_t)k0);
                child = a.out;
            }
        }
        // the cap's layers below the block roots, then the witness nodes it holds
        if (full)
            for (uint32_t l = b; l-- > 0;)
                hipLaunchKernelGGL(rsv::k_dc_cap_level, dim3(grid_for(Pc << l, 256)), dim3(256), 0, st, cap, cstride, l, (uint32_t)Pc, pl.cnt);
        hipLaunchKernelGGL(rsv::k_dc_gather_cap, dim3(grid_for(Pc * nq * b * 8, 256)), dim3(256), 0, st, cap, cstride, pl, out, (uint32_t)Pc);
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

}  // namespace

extern "C" {

int rsv_decommit_sizes(const rsv_commit_group* groups, size_t n_groups, uint32_t log_blowup, uint32_t n_queries, size_t* values_cap,
                       size_t* witness_cap) {
    if (!groups || !values_cap || !witness_cap) return RSV_E_NULL;
    if (n_groups == 0 || n_groups > RSV_MAX_COMMIT_GROUPS || log_blowup < 1 || log_blowup > RSV_MAX_LOG_BLOWUP || n_queries < 1 ||
        n_queries > RSV_MAX_QUERIES)
        return RSV_E_SIZE;
    for (size_t i = 0; i < n_groups; i++)
        if (groups[i].n_cols == 0 || groups[i].log_size + log_blowup > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;
    uint32_t top;
    decommit_caps(groups, n_groups, log_blowup, n_queries, &top, values_cap, witness_cap);
    return RSV_OK;
}

int rsv_decommit_tree_dev(rsv_ctx* c, const rsv_commit_group* groups, size_t n_groups, size_t n, uint32_t log_blowup, const uint8_t* d_mask,
                          const uint32_t* d_queries, uint32_t n_queries, int cap_mode, uint32_t* d_cap, uint32_t* d_values,
                          uint32_t* d_n_values, uint32_t* d_witness, uint32_t* d_n_witness) {
    if (!groups) return RSV_E_NULL;
    uint32_t top = 0;
    size_t vcap = 0, wcap = 0;
    if (n_groups >= 1 && n_groups <= RSV_MAX_COMMIT_GROUPS) decommit_caps(groups, n_groups, log_blowup, n_queries, &top, &vcap, &wcap);
    return decommit_tree(c, groups, n_groups, n, log_blowup, d_mask, d_queries, n_queries, cap_mode, d_cap, (uint64_t)16 << (log_blowup & 31),
                         d_values, vcap, d_n_values, d_witness, wcap * 8, d_n_witness, 1);
}

int rsv_witness_decommit_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                             const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept,
                             const uint8_t* d_ok, size_t n, uint32_t log_blowup, const uint32_t* d_queries, uint32_t n_queries,
                             const uint32_t* d_caps, uint32_t* d_values, uint32_t* d_n_values, uint32_t* d_witness, uint32_t* d_n_witness) {
    const ChainArgs a{c, prog, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, d_ok, n, log_blowup};
    if (chain_null(a, d_queries, d_values, d_n_values, d_witness, d_n_witness)) return RSV_E_NULL;
    if (log_blowup < 1 || log_blowup > RSV_MAX_LOG_BLOWUP || n_queries < 1 || n_queries > RSV_MAX_QUERIES) return RSV_E_SIZE;
    if (chain_misaligned(a, d_queries, d_caps, d_values, d_n_values, d_witness, d_n_witness)) return RSV_E_SIZE;
    ChainTrees ct;
    int rc = chain_open(a, &ct);
    if (rc != RSV_OK || n == 0) return rc;
    uint32_t top;
    size_t vcap[3], wcap, vall = 0;
    for (int t = 0; t < 3; t++) {
        decommit_caps(ct.tree(t), CHAIN_TREE_GROUPS[t], log_blowup, n_queries, &top, &vcap[t], &wcap);
        vall += vcap[t];
    }
    const uint64_t cap1 = (uint64_t)16 << log_blowup;
    size_t voff = 0;
    for (int t = 0; t < 3; t++) {
        rc = decommit_tree(c, ct.tree(t), CHAIN_TREE_GROUPS[t], n, log_blowup, ct.mask, d_queries, n_queries,
                           d_caps ? RSV_CAP_READ : RSV_CAP_NONE, d_caps ? const_cast<uint32_t*>(d_caps) + t * cap1 : nullptr, 3 * cap1,
                           d_values + voff, vall, d_n_values + t, d_witness + t * wcap * 8, 3 * wcap * 8, d_n_witness + t, 3);
        if (rc != RSV_OK) return rc;
        voff += vcap[t];
    }
    return RSV_OK;
}

}  // extern "C"
