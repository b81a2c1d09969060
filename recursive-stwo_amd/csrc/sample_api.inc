// sample_api.inc — rsv_sample_tree_dev (the sampled values of a tree's columns at up to RSV_MAX_SAMPLE_POINTS points per
// proof) and rsv_witness_sample_dev (sampled_values[0..2] of the recursion circuit's next proof, in the proof's own
// order): k_sample.hpp, include/rsv.h.  Included at the end of rsv_hip.hip, after decommit_api.inc.
//
// The driver has one path switch: a column of at most 2^SP_CHUNK_LOG = 2^13 rows is one workgroup of k_sp_dot, a larger
// one 2^(log - 13) of them, whose sums k_sp_finish adds.  Inside the kernel a column below 2^8 rows leaves lanes idle and
// one below 2^10 takes the loop without the four-way unrolling.  Pass sizing, tables and the interpolation are
// commit_api.inc's streaming helpers; there are no blocks, a pass is P proofs.

namespace {

// What one group is sampled at and where its values go.
struct SpGroup {
    rsv::SpPoints pts;
    uint32_t np;  // tables (points) per proof
    rsv::SpOut out;
};

struct SpWs {
    uint32_t *coef[RSV_MAX_COMMIT_GROUPS], *wt[RSV_MAX_COMMIT_GROUPS], *part[RSV_MAX_COMMIT_GROUPS];
};

// The group whose weight tables group i shares: the first one of the same size sampled at the same points.
size_t sp_table_of(const rsv_commit_group* g, const SpGroup* sg, size_t i) {
    for (size_t j = 0; j < i; j++)
        if (g[j].log_size == g[i].log_size && sg[j].pts.pts == sg[i].pts.pts && sg[j].pts.np_in == sg[i].pts.np_in &&
            sg[j].pts.prev_log == sg[i].pts.prev_log && sg[j].np == sg[i].np)
            return j;
    return i;
}

// Workspace of a pass of P proofs: the coefficients (from evaluations only), the weight tables, the chunk sums.
size_t sp_ws_bytes(const rsv_commit_group* g, const SpGroup* sg, size_t ng, bool interpolate, size_t P, char* base, SpWs* w) {
    rsv::host::Carve sz{base};
    SpWs t{};
    for (size_t i = 0; i < ng; i++) {
        const uint32_t log = g[i].log_size;
        const size_t chunks = (size_t)1 << (log > rsv::SP_CHUNK_LOG ? log - rsv::SP_CHUNK_LOG : 0);
        t.coef[i] = interpolate ? sz.take<uint32_t>(P * g[i].n_cols << log) : nullptr;
        const size_t j = sp_table_of(g, sg, i);
        t.wt[i] = j < i ? t.wt[j] : sz.take<uint32_t>(P * sg[i].np * rsv::sp_table_entries(log) * 4);
        t.part[i] = sz.take<uint32_t>(P * g[i].n_cols * sg[i].np * chunks * 4);
    }
    if (w) *w = t;
    return sz.off;
}

template <uint32_t NP>
void sp_dot(hipStream_t st, unsigned grid, const rsv::SpCols& s, const uint32_t* wt, uint32_t* part) {
    hipLaunchKernelGGL(rsv::k_sp_dot<NP>, dim3(grid), dim3(256), 0, st, s, wt, part);
}

int sample_groups(rsv_ctx* c, const rsv_commit_group* g, size_t ng, size_t n, const uint8_t* d_mask, int source, const SpGroup* sg) {
    if (ng == 0 || ng > RSV_MAX_COMMIT_GROUPS || n > (1u << 20)) return RSV_E_SIZE;
    if (source != RSV_SAMPLE_COLUMNS && source != RSV_SAMPLE_COEFFS) return RSV_E_SIZE;
    for (size_t i = 0; i < ng; i++) {
        if (!g[i].d_cols) return RSV_E_NULL;
        if (g[i].n_cols == 0 || g[i].log_size >= RSV_MAX_LOG_SIZE || ((uintptr_t)g[i].d_cols & 3)) return RSV_E_SIZE;
    }
    if (n == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    const bool interpolate = source == RSV_SAMPLE_COLUMNS;
    const auto ws = [&](size_t P, size_t, char* base = nullptr, SpWs* w = nullptr) { return sp_ws_bytes(g, sg, ng, interpolate, P, base, w); };
    const size_t P = rsv::host::plan_pass(ws_budget(c), n, 1, ws).P;
    for (size_t i = 0; i < ng; i++) {
        const uint32_t log = g[i].log_size;
        if (!cm_rows_fit((uint64_t)P * g[i].n_cols, log) || (uint64_t)P * sg[i].np * rsv::sp_table_entries(log) / 256 >= CM_GRID_LIM) return RSV_E_SIZE;
    }
    const uint32_t* tw_inv[RSV_MAX_COMMIT_GROUPS] = {};
    int rc = cm_group_twiddles(c, g, ng, 0, interpolate ? tw_inv : nullptr, nullptr);
    SpWs w;
    if (rc == RSV_OK) rc = cm_workspace(c, [&](char* base) { return ws(P, 1, base, &w); });
    if (rc != RSV_OK) return rc;
    hipStream_t st = c->stream;
    for (size_t p0 = 0; p0 < n; p0 += P) {
        const size_t Pc = std::min(P, n - p0);
        for (size_t i = 0; i < ng; i++) {
            const uint32_t log = g[i].log_size, cols = g[i].n_cols, np = sg[i].np;
            const size_t row = (size_t)1 << log;
            const uint32_t clog = log > rsv::SP_CHUNK_LOG ? log - rsv::SP_CHUNK_LOG : 0;
            if (sp_table_of(g, sg, i) == i)
                hipLaunchKernelGGL(rsv::k_sp_weights, dim3(grid_for(Pc * np * rsv::sp_table_entries(log), 256)), dim3(256), 0, st, sg[i].pts, np, log,
                                   (uint32_t)p0, (uint32_t)Pc, w.wt[i]);
            rsv::SpCols s{g[i].d_cols + p0 * g[i].proof_stride, g[i].proof_stride, row, d_mask, (uint32_t)p0, cols, log};
            if (interpolate) {
                cm_interpolate(st, g[i], w.coef[i], p0, Pc, d_mask, false, tw_inv[i]);
                s.base = w.coef[i];
                s.pstride = (uint64_t)cols * row;
            }
            const unsigned grid = (unsigned)(((uint64_t)Pc * cols) << clog);
            switch (np) {
                case 1: sp_dot<1>(st, grid, s, w.wt[i], w.part[i]); break;
                case 2: sp_dot<2>(st, grid, s, w.wt[i], w.part[i]); break;
                case 3: sp_dot<3>(st, grid, s, w.wt[i], w.part[i]); break;
                default: sp_dot<4>(st, grid, s, w.wt[i], w.part[i]); break;
            }
            hipLaunchKernelGGL(rsv::k_sp_finish, dim3(grid_for(Pc * cols * np, 256)), dim3(256), 0, st, w.part[i], np, cols, log, (uint32_t)Pc,
                               d_mask, (uint32_t)p0, sg[i].out);
        }
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

}  // namespace

extern "C" {

int rsv_sample_tree_dev(rsv_ctx* c, const rsv_commit_group* groups, size_t n_groups, size_t n, const uint8_t* d_mask, int source,
                        const uint32_t* d_points, uint32_t n_points, uint32_t* d_samples) {
    if (!c || !groups || !d_points || !d_samples) return RSV_E_NULL;
    if (n_points < 1 || n_points > RSV_MAX_SAMPLE_POINTS || n_groups == 0 || n_groups > RSV_MAX_COMMIT_GROUPS) return RSV_E_SIZE;
    if (((uintptr_t)d_points & 3) || ((uintptr_t)d_samples & 3)) return RSV_E_SIZE;
    SpGroup sg[RSV_MAX_COMMIT_GROUPS];
    uint64_t total = 0;
    for (size_t i = 0; i < n_groups; i++) total += groups[i].n_cols;
    if (total > 0xffffffffu) return RSV_E_SIZE;
    uint32_t col0 = 0;
    for (size_t i = 0; i < n_groups; i++) {
        sg[i] = {{d_points, n_points, 0}, n_points, {d_samples, (uint64_t)n_points * total * 4, col0, (uint32_t)total, 0, 0}};
        col0 += groups[i].n_cols;
    }
    return sample_groups(c, groups, n_groups, n, d_mask, source, sg);
}

int rsv_witness_sample_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                           const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept,
                           const uint8_t* d_ok, size_t n, const uint32_t* d_oods, uint32_t* d_samples) {
    const ChainArgs a{c, prog, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, d_ok, n, 0};
    if (chain_null(a, d_oods, d_samples)) return RSV_E_NULL;
    if (chain_misaligned(a, d_oods, d_samples)) return RSV_E_SIZE;
    ChainTrees ct;
    int rc = chain_open(a, &ct);
    if (rc != RSV_OK || n == 0) return rc;
    // One call per tree.  A group that CHAIN_SAMPLES cuts is sampled whole at two points: its first columns take the OODS
    // value alone, the cumulative ones the previous-row value and then the OODS value.  That is the table's row of the
    // cumulative half (entry + cols + 1, step 2: the table's static_assert), so the row itself has nothing left to place.
    SpGroup sg[3][4];
    for (const ChainSamples& s : CHAIN_SAMPLES) {
        if (s.col0) continue;
        const rsv_commit_group& g = ct.tree(s.tree)[s.group];
        const bool cut = s.cols < g.n_cols;
        sg[s.tree][s.group] = {{d_oods, 1, cut ? g.log_size : 0}, cut ? 2u : 1u, {d_samples, CHAIN_SAMPLE_VALUES * 4, s.entry, 0, cut ? s.cols : 0, 1}};
    }
    for (int t = 0; t < 3; t++) {
        rc = sample_groups(c, ct.tree(t), CHAIN_TREE_GROUPS[t], n, ct.mask, RSV_SAMPLE_COLUMNS, sg[t]);
        if (rc != RSV_OK) return rc;
    }
    return RSV_OK;
}

}  // extern "C"
