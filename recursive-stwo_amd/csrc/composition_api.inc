// composition_api.inc — rsv_composition_dev (tree 3's eight columns: the composition polynomial of the recursion
// circuit's two components, cut into left and right) and rsv_witness_tree3_dev (those columns from the chain's buffers,
// their commitment, the OODS point drawn behind root 3 and the eight sampled values at it): k_composition.hpp,
// include/rsv.h.  Included at the end of rsv_hip.hip, after sample_api.inc.
//
// The driver streams the extended domain of 2^clb rows in aligned blocks of 2^(max(lp, lq) + 1) rows, the smallest that
// hold every row's previous-row neighbour of both components (k_composition.hpp); a pass holds nc of them for P proofs.
// The accumulator's values of the whole domain stay in the workspace (4 x 2^clb words per proof), are interpolated in
// place, cut, and evaluated on the domain 2^(clb - 1).  The groups' passes, interpolation and extension are commit_api.inc's
// streaming helpers (a block of theirs is 2^log rows of a group); the accumulator's and the output's FFTs are the driver's own.

namespace {

// Host arithmetic shared by the entry points: clb = max(lp + 2, lq + 3).
uint32_t co_clb(uint32_t lp, uint32_t lq) { return std::max(lp + 2, lq + 3); }

struct CoWs {
    uint32_t *coef[RSV_MAX_COMMIT_GROUPS], *ext[RSV_MAX_COMMIT_GROUPS], *par, *zinv[2], *acc, *cut;
};

// Workspace of a pass of P proofs and nc blocks: per group the coefficients and the extended rows of the blocks in
// flight (one set for a shared group), the per-proof parameters, the two 1/Z tables, the accumulator's values on the
// whole domain and, without d_comp_coeffs, the cut coefficients.
size_t co_ws_bytes(const rsv_commit_group* g, size_t ng, uint32_t lp, uint32_t lq, size_t P, size_t nc, bool cut, char* base, CoWs* w) {
    rsv::host::Carve sz{base};
    CoWs t{};
    const uint32_t clb = co_clb(lp, lq);
    const size_t R = nc << (std::max(lp, lq) + 1);
    for (size_t i = 0; i < ng; i++) {
        const size_t np = g[i].proof_stride ? P : 1;
        t.coef[i] = sz.take<uint32_t>(np * g[i].n_cols << g[i].log_size);
        t.ext[i] = sz.take<uint32_t>(np * g[i].n_cols * R);
    }
    t.par = sz.take<uint32_t>(P * rsv::CO_PARAM_Q * 4);
    t.zinv[0] = sz.take<uint32_t>((size_t)1 << (clb - lp));
    t.zinv[1] = sz.take<uint32_t>((size_t)1 << (clb - lq));
    t.acc = sz.take<uint32_t>((P * 4) << clb);
    t.cut = cut ? sz.take<uint32_t>((P * 4) << clb) : nullptr;
    if (w) *w = t;
    return sz.off;
}

// g: the Plonk component's n_plonk groups (columns in component order: 10 preprocessed, 12 trace, 8 interaction), then
// the Poseidon component's (40, 48, 8), at log sizes lp and lq.
int composition(rsv_ctx* c, const rsv_commit_group* g, size_t n_plonk, size_t ng, uint32_t lp, uint32_t lq, size_t n, const uint32_t* d_sums,
                const uint32_t* d_draws, const uint8_t* d_mask, uint32_t* d_comp, uint32_t* d_comp_coeffs) {
    const uint32_t clb = co_clb(lp, lq), L3 = clb - 1, Lb = std::max(lp, lq);
    if (n == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    const bool cut = !d_comp_coeffs;
    const auto ws = [&](size_t P, size_t nc, char* base = nullptr, CoWs* w = nullptr) { return co_ws_bytes(g, ng, lp, lq, P, nc, cut, base, w); };
    const rsv::host::Pass pass = rsv::host::plan_pass(ws_budget(c), n, (size_t)1 << (clb - Lb - 1), ws);
    const size_t P = pass.P, nc = pass.nb, R = nc << (Lb + 1);
    uint32_t rlog = 0;
    while (((size_t)1 << rlog) < R) rlog++;
    for (size_t i = 0; i < ng; i++)
        if (!cm_rows_fit((uint64_t)P * g[i].n_cols * (R >> g[i].log_size), g[i].log_size)) return RSV_E_SIZE;
    if ((((uint64_t)P * 8) << L3) / 256 >= CM_GRID_LIM || (uint64_t)P * std::max<size_t>(R / 256, 1) >= CM_GRID_LIM) return RSV_E_SIZE;
    const uint32_t *tw_inv[RSV_MAX_COMMIT_GROUPS], *tw_ext, *tw_acc, *tw_out;
    int rc = cm_twiddles(c, clb, false, &tw_ext);
    if (rc == RSV_OK) rc = cm_twiddles(c, clb, true, &tw_acc);
    if (rc == RSV_OK) rc = cm_twiddles(c, L3, false, &tw_out);
    if (rc == RSV_OK) rc = cm_group_twiddles(c, g, ng, 0, tw_inv, nullptr);
    CoWs w;
    if (rc == RSV_OK) rc = cm_workspace(c, [&](char* base) { return ws(P, nc, base, &w); });
    if (rc != RSV_OK) return rc;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(rsv::k_co_zinv, dim3(grid_for((size_t)1 << (clb - lp), 256)), dim3(256), 0, st, clb, lp, w.zinv[0]);
    hipLaunchKernelGGL(rsv::k_co_zinv, dim3(grid_for((size_t)1 << (clb - lq), 256)), dim3(256), 0, st, clb, lq, w.zinv[1]);
    for (size_t p0 = 0; p0 < n; p0 += P) {
        const size_t Pc = std::min(P, n - p0);
        hipLaunchKernelGGL(rsv::k_co_params, dim3(grid_for(Pc, 64)), dim3(64), 0, st, d_draws, d_sums, d_mask, (uint32_t)p0, (uint32_t)Pc, lp, lq,
                           w.par);
        for (size_t i = 0; i < ng; i++) cm_interpolate(st, g[i], w.coef[i], p0, Pc, d_mask, true, tw_inv[i]);
        for (size_t row0 = 0; row0 < ((size_t)1 << clb); row0 += R) {
            // the extension of the rows row0 .. row0 + R - 1: R >> log blocks of every column
            rsv::CoRows a[2] = {};
            for (size_t i = 0; i < ng; i++) {
                const uint32_t log = g[i].log_size, cols = g[i].n_cols;
                const size_t np = g[i].proof_stride ? Pc : 1;
                cm_extend(st, g[i], w.coef[i], (uint64_t)cols << log, np * cols, clb, R >> log, row0 >> log, {w.ext[i], R}, tw_ext);
                rsv::CoRows& k = a[i < n_plonk ? 0 : 1];
                const uint32_t col0 = k.n_parts ? k.part[k.n_parts - 1].col0 + g[i - 1].n_cols : 0;
                k.part[k.n_parts++] = {w.ext[i], g[i].proof_stride ? (uint64_t)cols * R : 0, col0};
            }
            for (int k = 0; k < 2; k++) {
                a[k].log = k ? lq : lp;
                a[k].rlog = rlog;
                a[k].row0 = row0;
                a[k].par = w.par;
                a[k].zinv = w.zinv[k];
                a[k].mask = d_mask;
                a[k].p0 = (uint32_t)p0;
                a[k].clb = clb;
                a[k].acc = w.acc;
            }
            const dim3 grid((unsigned)(Pc * std::max<size_t>(R / 256, 1)));
            hipLaunchKernelGGL(rsv::k_co_plonk, grid, dim3(256), 0, st, a[0]);
            hipLaunchKernelGGL(rsv::k_co_poseidon, grid, dim3(256), 0, st, a[1]);
        }
        // the four coordinates' coefficients in place (masked proofs zero), the cut, the eight halves on the domain 2^L3
        rsv::CmRows ra{w.acc, (uint64_t)1 << clb, (uint64_t)Pc * 4, clb, clb, 1, 0};
        rsv::CmSrc sa{w.acc, (uint64_t)4 << clb, (uint64_t)1 << clb, d_mask, 4, (uint32_t)p0, 1u << (31 - clb)};
        cm_fft<true>(st, ra, sa, tw_acc);
        uint32_t* halves = cut ? w.cut : d_comp_coeffs + ((p0 * 8) << L3);
        hipLaunchKernelGGL(rsv::k_co_cut, dim3(grid_for((Pc * 8) << L3, 256)), dim3(256), 0, st, w.acc, L3, (uint32_t)Pc, halves);
        rsv::CmRows ro{d_comp + ((p0 * 8) << L3), (uint64_t)1 << L3, (uint64_t)Pc * 8, L3, L3, 1, 0};
        rsv::CmSrc so{halves, (uint64_t)8 << L3, (uint64_t)1 << L3, nullptr, 8, 0, 1};
        cm_fft<false>(st, ro, so, tw_out);
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int co_check_sizes(uint32_t lp, uint32_t lq, size_t n) {
    if (lp < 2 || lq < 2 || lp > RSV_MAX_LOG_SIZE || lq > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;  // as rsv_witness_interaction_dev
    if (co_clb(lp, lq) > RSV_MAX_LOG_SIZE || n > (1u << 20)) return RSV_E_SIZE;
    return RSV_OK;
}

}  // namespace

extern "C" {

int rsv_composition_log_size(uint32_t lp, uint32_t lq, uint32_t* log_size) {
    if (!log_size) return RSV_E_NULL;
    const int rc = co_check_sizes(lp, lq, 0);
    if (rc != RSV_OK) return rc;
    *log_size = co_clb(lp, lq) - 1;
    return RSV_OK;
}

int rsv_composition_dev(rsv_ctx* c, uint32_t lp, uint32_t lq, const uint32_t* d_plonk_pre, uint64_t plonk_pre_stride, const uint32_t* d_plonk,
                        uint64_t plonk_stride, const uint32_t* d_int_plonk, uint64_t int_plonk_stride, const uint32_t* d_poseidon_pre,
                        uint64_t poseidon_pre_stride, const uint32_t* d_poseidon, uint64_t poseidon_stride, const uint32_t* d_int_poseidon,
                        uint64_t int_poseidon_stride, const uint32_t* d_sums, const uint32_t* d_draws, const uint8_t* d_mask, size_t n,
                        uint32_t* d_comp, uint32_t* d_comp_coeffs) {
    if (!c || !d_plonk_pre || !d_plonk || !d_int_plonk || !d_poseidon_pre || !d_poseidon || !d_int_poseidon || !d_sums || !d_draws || !d_comp)
        return RSV_E_NULL;
    const int rc = co_check_sizes(lp, lq, n);
    if (rc != RSV_OK) return rc;
    if (((uintptr_t)d_plonk_pre & 3) || ((uintptr_t)d_plonk & 3) || ((uintptr_t)d_int_plonk & 3) || ((uintptr_t)d_poseidon_pre & 3) ||
        ((uintptr_t)d_poseidon & 3) || ((uintptr_t)d_int_poseidon & 3) || ((uintptr_t)d_sums & 3) || ((uintptr_t)d_draws & 3) ||
        ((uintptr_t)d_comp & 3) || ((uintptr_t)d_comp_coeffs & 3))
        return RSV_E_SIZE;
    const rsv_commit_group g[6] = {{lp, rsv::trace::PLONK_PRE_COLS, d_plonk_pre, plonk_pre_stride, nullptr, nullptr},
                                   {lp, rsv::PLONK_COLS_K, d_plonk, plonk_stride, nullptr, nullptr},
                                   {lp, rsv::INT_COLS, d_int_plonk, int_plonk_stride, nullptr, nullptr},
                                   {lq, rsv::trace::POSEIDON_PRE_COLS, d_poseidon_pre, poseidon_pre_stride, nullptr, nullptr},
                                   {lq, rsv::POSEIDON_COLS_K, d_poseidon, poseidon_stride, nullptr, nullptr},
                                   {lq, rsv::INT_COLS, d_int_poseidon, int_poseidon_stride, nullptr, nullptr}};
    return composition(c, g, 3, 6, lp, lq, n, d_sums, d_draws, d_mask, d_comp, d_comp_coeffs);
}

int rsv_witness_tree3_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                          const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept,
                          const uint8_t* d_ok, size_t n, uint32_t log_blowup, const uint32_t* d_sums, const uint32_t* d_draws,
                          uint32_t* d_channel, uint32_t* d_comp, uint32_t* d_root3, uint32_t* d_cap3, uint32_t* d_oods, uint32_t* d_samples3) {
    const ChainArgs a{c, prog, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, d_ok, n, 0};
    if (chain_null(a, d_sums, d_draws, d_channel, d_comp, d_root3, d_oods, d_samples3)) return RSV_E_NULL;
    if (log_blowup < 1 || log_blowup > RSV_MAX_LOG_BLOWUP) return RSV_E_SIZE;
    if (chain_misaligned(a, d_sums, d_draws, d_channel, d_comp, d_root3, d_cap3, d_oods, d_samples3)) return RSV_E_SIZE;
    if (prog->gates.empty()) return RSV_E_SIZE;  // built programs only
    const uint32_t lp = prog->trace_lp, lq = prog->trace_lq;
    int rc = co_check_sizes(lp, lq, n);
    if (rc != RSV_OK) return rc;
    const uint32_t L3 = co_clb(lp, lq) - 1;
    if (L3 + log_blowup > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;
    ChainTrees ct;
    rc = chain_open(a, &ct);
    if (rc != RSV_OK || n == 0) return rc;
    const uint8_t* mask = ct.mask;
    // the components' columns in component order: preprocessed (the op column is the proof's own), trace, interaction
    const rsv_commit_group g[8] = {ct.t0[0], ct.t0[1], ct.t0[2], ct.t1[0], ct.t2[0], ct.t0[3], ct.t1[1], ct.t2[1]};
    rc = composition(c, g, 5, 8, lp, lq, n, d_sums, d_draws, mask, d_comp, nullptr);
    if (rc != RSV_OK) return rc;
    const rsv_commit_group t3{L3, 8, d_comp, (uint64_t)8 << L3, nullptr, nullptr};
    rc = commit_tree(c, &t3, 1, n, log_blowup, mask, d_root3, 8, d_cap3, (uint64_t)16 << log_blowup);
    if (rc != RSV_OK) return rc;
    hipLaunchKernelGGL(rsv::k_co_draw_oods, dim3(grid_for(n, 64)), dim3(64), 0, c->stream, d_root3, mask, (uint32_t)n, d_channel, d_oods);
    const SpGroup sg{{d_oods, 1, 0}, 1, {d_samples3, 8 * 4, 0, 8, 0, 0}};
    return sample_groups(c, &t3, 1, n, mask, RSV_SAMPLE_COLUMNS, &sg);
}

}  // extern "C"
