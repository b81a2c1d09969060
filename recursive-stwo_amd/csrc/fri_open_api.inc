// fri_open_api.inc — rsv_fri_open_sizes, rsv_fri_open_dev and rsv_fri_open_cap_dev (the openings of the FRI layer trees at a
// list of positions: fri_witness and hash_witness in stwo's pair-tree order): k_fri_open.hpp, include/rsv.h.  Included at the
// end of rsv_hip.hip, after pow_api.inc.
//
// The recompute form: fri_commit keeps the roots only, so every tree is hashed again level by level (k_fr_hash_layer through
// the same two node buffers), and k_fo_gather copies the nodes the plan names while their level is still in a buffer.
// The cap form: rsv_fri_commit_cap_dev kept the top of every tree, so only the subtrees that hold a planned node are
// hashed, each by one workgroup in LDS, and the planned nodes above them are read from the cap: six launches whatever M is.

namespace {

// Capacities per (proof, tree).  Values: a data layer gives at most one value per query (the sibling of a queried node
// nobody else queries).  Nodes, by the level l = top - 1 .. 0 whose set S_l asks for its children:
//   a level without data asks for at most one child per node of Q_l:                       n_queries;
//   a data level below the top asks, per node of Q_(l-1), for at most one child of a queried node and both children of
//   a sibling nobody queries:                                                            3 n_queries;
//   (the level under a data level asks for nothing from the queried parents' own pair: S_(l+1) holds both.)
// M levels of which n_sizes - 1 are data levels below the top: n_queries (M + 2 (n_sizes - 1)); an inner layer's tree has
// fewer levels and no data level below its top.
void fri_open_caps(const uint32_t* sizes, size_t ns, uint32_t nq, size_t* vcap, size_t* wcap) {
    *vcap = ns * nq;
    *wcap = (size_t)nq * (sizes[0] + 2 * (ns - 1));
}

struct FoWs {
    uint32_t *na, *nb;
    rsv::FoPlan pl;
};
// Workspace of an opening: the plan of all n proofs' trees, and two node layers of a pass of P proofs.
rsv::FoPlan fo_carve_plan(rsv::host::Carve& sz, uint32_t M, uint32_t T, size_t n, uint32_t nq, size_t vcap, size_t wcap) {
    rsv::FoPlan pl{};
    pl.woff = sz.take<uint32_t>(n * T * rsv::DC_LAYERS);
    pl.wnode = sz.take<uint32_t>(n * T * wcap);
    pl.vnode = sz.take<uint32_t>(n * T * vcap);
    pl.vlayer = sz.take<uint32_t>(n * T * vcap);
    pl.T = T;
    pl.M = M;
    pl.nq = nq;
    pl.wcap = (uint32_t)wcap;
    pl.vcap = (uint32_t)vcap;
    return pl;
}
size_t fo_ws_bytes(uint32_t M, uint32_t T, size_t n, uint32_t nq, size_t vcap, size_t wcap, size_t P, char* base, FoWs* w) {
    rsv::host::Carve sz{base};
    FoWs t{};
    t.pl = fo_carve_plan(sz, M, T, n, nq, vcap, wcap);
    t.na = sz.take<uint32_t>((P * 8) << M);
    t.nb = sz.take<uint32_t>((P * 8) << (M - 1));
    if (w) *w = t;
    return sz.off;
}

// The plan's view from proof p0 on.
rsv::FoPlan fo_plan_at(rsv::FoPlan pl, size_t p0) {
    pl.woff += p0 * pl.T * rsv::DC_LAYERS;
    pl.wnode += p0 * pl.T * pl.wcap;
    pl.vnode += p0 * pl.T * pl.vcap;
    pl.vlayer += p0 * pl.T * pl.vcap;
    return pl;
}

// Where the values of the trees live, and (-> the bits) which layers of tree 0 carry one.
uint32_t fo_data(const uint32_t* d_quot, const uint32_t* d_layers, const uint32_t* sizes, size_t ns, uint32_t n_inner, rsv::FoData* data) {
    *data = rsv::FoData{d_quot, d_layers, 0, 0, {}};
    uint32_t dmask = 0;
    for (size_t s = 0; s < ns; s++) {
        data->col_at[sizes[s]] = data->qstride;
        data->qstride += (uint64_t)4 << sizes[s];
        dmask |= 1u << sizes[s];
    }
    for (uint32_t i = 0; i < n_inner; i++) data->lstride += (uint64_t)4 << (sizes[0] - 1 - i);
    return dmask;
}

int fri_open(rsv_ctx* c, const uint32_t* d_quot, const uint32_t* d_layers, const uint32_t* sizes, size_t ns, uint32_t b, uint32_t log_last, size_t n,
             const uint8_t* d_mask, const uint32_t* d_queries, uint32_t nq, uint32_t* d_fri_witness, uint32_t* d_n_fri_witness,
             uint32_t* d_hash_witness, uint32_t* d_n_hash_witness) {
    if (n == 0) return RSV_OK;
    const uint32_t M = sizes[0], n_inner = M - 1 - log_last - b, T = 1 + n_inner;
    size_t vcap, wcap;
    fri_open_caps(sizes, ns, nq, &vcap, &wcap);
    rsv::FoData data;
    const uint32_t dmask = fo_data(d_quot, d_layers, sizes, ns, n_inner, &data);
    HIP_TRY(hipSetDevice(c->device));
    const auto ws = [&](size_t P, size_t, char* base = nullptr, FoWs* w = nullptr) { return fo_ws_bytes(M, T, n, nq, vcap, wcap, P, base, w); };
    const size_t P = rsv::host::plan_pass(ws_budget(c), n, 1, ws).P;
    if (((uint64_t)P << M) / 256 >= CM_GRID_LIM || ((uint64_t)n * T * std::max(vcap * 4, wcap * 8)) / 256 >= CM_GRID_LIM) return RSV_E_SIZE;
    FoWs w;
    const int rc = cm_workspace(c, [&](char* base) { return ws(P, 1, base, &w); });
    if (rc != RSV_OK) return rc;
    w.pl.dmask = dmask;
    hipStream_t st = c->stream;
    // every element of the outputs is defined: the witness nodes zero, then the planned ones; the values in one launch
    hipLaunchKernelGGL(rsv::k_dc_zero, dim3(grid_for(n * T * wcap * 8, 256)), dim3(256), 0, st, d_hash_witness, (uint64_t)T * wcap * 8,
                       (uint64_t)T * wcap * 8, (uint64_t)n);
    hipLaunchKernelGGL(rsv::k_fo_plan, dim3((unsigned)n, T), dim3(128), 0, st, d_queries, d_mask, w.pl, d_n_fri_witness, d_n_hash_witness);
    hipLaunchKernelGGL(rsv::k_fo_values, dim3(grid_for(n * T * vcap * 4, 256)), dim3(256), 0, st, data, w.pl, d_n_fri_witness, (uint32_t)n,
                       d_fri_witness);
    for (size_t p0 = 0; p0 < n; p0 += P) {
        const uint32_t Pc = (uint32_t)std::min(P, n - p0);
        const rsv::FoPlan pl = fo_plan_at(w.pl, p0);
        uint32_t* out = d_hash_witness + p0 * T * wcap * 8;
        // tree t: fri_commit's levels (fr_tree) top .. 1, the root being nobody's witness; the two node buffers hold two
        // levels, so the planned nodes are taken after every second level (l + 1 in na, l in nb), and after the last
        const dim3 grid(grid_for((size_t)Pc * 6 * nq * 8, 256));
        for (uint32_t t = 0; t < T; t++) {
            const uint32_t top = M - t;
            fr_tree(
                st, Pc, top, 1, w.na, w.nb, nullptr,
                [&](uint32_t l, uint64_t* stride) -> const uint32_t* {
                    if (t == 0) {
                        *stride = data.qstride;
                        return dmask >> l & 1u ? d_quot + p0 * data.qstride + data.col_at[l] : nullptr;
                    }
                    *stride = data.lstride;
                    return l == top ? d_layers + p0 * data.lstride + rsv::fr_layer_off(M, l) : nullptr;
                },
                fr_keep_none,
                [&](uint32_t l, const uint32_t*) {
                    if ((top - l) & 1) hipLaunchKernelGGL(rsv::k_fo_gather, grid, dim3(256), 0, st, w.na, w.nb, l + 1, t, Pc, pl, out);
                    else if (l == 1) hipLaunchKernelGGL(rsv::k_fo_gather, grid, dim3(256), 0, st, w.na, nullptr, l, t, Pc, pl, out);
                });
        }
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

struct FoCapWs {
    rsv::FoPlan pl;
    rsv::FoSubs sb;
};
// Workspace of a capped opening: the plan and the subtree lists of all n proofs' trees; there are no node buffers.
size_t fo_cap_ws_bytes(uint32_t M, uint32_t T, size_t n, uint32_t nq, size_t vcap, size_t wcap, char* base, FoCapWs* w) {
    rsv::host::Carve sz{base};
    FoCapWs t{};
    t.pl = fo_carve_plan(sz, M, T, n, nq, vcap, wcap);
    t.sb.cnt = sz.take<uint32_t>(n * T);
    t.sb.ids = sz.take<uint32_t>(n * T * 2 * nq);
    if (w) *w = t;
    return sz.off;
}

int fri_open_cap(rsv_ctx* c, const uint32_t* d_quot, const uint32_t* d_layers, const uint32_t* sizes, size_t ns, uint32_t b, uint32_t log_last,
                 size_t n, const uint8_t* d_mask, const uint32_t* d_queries, uint32_t nq, uint32_t* d_fri_witness, uint32_t* d_n_fri_witness,
                 uint32_t* d_hash_witness, uint32_t* d_n_hash_witness, uint32_t sub_log, const uint32_t* d_caps) {
    if (n == 0) return RSV_OK;
    const uint32_t M = sizes[0], n_inner = M - 1 - log_last - b, T = 1 + n_inner;
    size_t vcap, wcap;
    fri_open_caps(sizes, ns, nq, &vcap, &wcap);
    rsv::FoData data;
    const uint32_t dmask = fo_data(d_quot, d_layers, sizes, ns, n_inner, &data);
    rsv::FoCaps caps{d_caps, {}, n, sub_log};
    fr_cap_words(M, n_inner, sub_log, n, caps.tree_at);
    HIP_TRY(hipSetDevice(c->device));
    // a workgroup per (proof, tree, subtree slot); a lane per word of the outputs
    if ((uint64_t)n * T * 2 * nq >= CM_GRID_LIM || ((uint64_t)n * T * std::max(vcap * 4, wcap * 8)) / 256 >= CM_GRID_LIM) return RSV_E_SIZE;
    FoCapWs w;
    const int rc = cm_workspace(c, [&](char* base) { return fo_cap_ws_bytes(M, T, n, nq, vcap, wcap, base, &w); });
    if (rc != RSV_OK) return rc;
    w.pl.dmask = dmask;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(rsv::k_dc_zero, dim3(grid_for(n * T * wcap * 8, 256)), dim3(256), 0, st, d_hash_witness, (uint64_t)T * wcap * 8,
                       (uint64_t)T * wcap * 8, (uint64_t)n);
    hipLaunchKernelGGL(rsv::k_fo_plan, dim3((unsigned)n, T), dim3(128), 0, st, d_queries, d_mask, w.pl, d_n_fri_witness, d_n_hash_witness);
    hipLaunchKernelGGL(rsv::k_fo_values, dim3(grid_for(n * T * vcap * 4, 256)), dim3(256), 0, st, data, w.pl, d_n_fri_witness, (uint32_t)n,
                       d_fri_witness);
    hipLaunchKernelGGL(rsv::k_fo_sublist, dim3((unsigned)n, T), dim3(128), 0, st, w.pl, sub_log, w.sb);
    hipLaunchKernelGGL(rsv::k_fo_subtree, dim3((unsigned)(n * T * 2 * nq)), dim3(256), 0, st, data, w.pl, sub_log, w.sb, d_hash_witness);
    hipLaunchKernelGGL(rsv::k_fo_cap_gather, dim3(grid_for(n * T * wcap * 8, 256)), dim3(256), 0, st, caps, w.pl, (uint32_t)n, d_hash_witness);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

}  // namespace

extern "C" {

int rsv_fri_open_sizes(const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup, uint32_t log_last, uint32_t n_queries, size_t* values_cap,
                       size_t* witness_cap) {
    if (!sizes || !values_cap || !witness_cap) return RSV_E_NULL;
    const int rc = fr_check_commit(sizes, n_sizes, log_blowup, log_last, 0);
    if (rc != RSV_OK) return rc;
    if (n_queries < 1 || n_queries > RSV_MAX_QUERIES) return RSV_E_SIZE;
    fri_open_caps(sizes, n_sizes, n_queries, values_cap, witness_cap);
    return RSV_OK;
}

int rsv_fri_open_dev(rsv_ctx* c, const uint32_t* d_quot, const uint32_t* d_layers, const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup,
                     uint32_t log_last, size_t n, const uint8_t* d_mask, const uint32_t* d_queries, uint32_t n_queries, uint32_t* d_fri_witness,
                     uint32_t* d_n_fri_witness, uint32_t* d_hash_witness, uint32_t* d_n_hash_witness) {
    if (!c || !d_quot || !sizes || !d_queries || !d_fri_witness || !d_n_fri_witness || !d_hash_witness || !d_n_hash_witness) return RSV_E_NULL;
    const int rc = fr_check_commit(sizes, n_sizes, log_blowup, log_last, n);
    if (rc != RSV_OK) return rc;
    if (!d_layers && sizes[0] - 1 - log_last - log_blowup > 0) return RSV_E_NULL;
    if (n_queries < 1 || n_queries > RSV_MAX_QUERIES) return RSV_E_SIZE;
    if (((uintptr_t)d_quot & 3) || ((uintptr_t)d_layers & 3) || ((uintptr_t)d_queries & 3) || ((uintptr_t)d_fri_witness & 3) ||
        ((uintptr_t)d_n_fri_witness & 3) || ((uintptr_t)d_hash_witness & 3) || ((uintptr_t)d_n_hash_witness & 3))
        return RSV_E_SIZE;
    return fri_open(c, d_quot, d_layers, sizes, n_sizes, log_blowup, log_last, n, d_mask, d_queries, n_queries, d_fri_witness, d_n_fri_witness,
                    d_hash_witness, d_n_hash_witness);
}

int rsv_fri_open_cap_dev(rsv_ctx* c, const uint32_t* d_quot, const uint32_t* d_layers, const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup,
                         uint32_t log_last, size_t n, const uint8_t* d_mask, const uint32_t* d_queries, uint32_t n_queries, uint32_t* d_fri_witness,
                         uint32_t* d_n_fri_witness, uint32_t* d_hash_witness, uint32_t* d_n_hash_witness, uint32_t sub_log, const uint32_t* d_caps) {
    if (!c || !d_quot || !sizes || !d_queries || !d_fri_witness || !d_n_fri_witness || !d_hash_witness || !d_n_hash_witness || !d_caps)
        return RSV_E_NULL;
    const int rc = fr_check_commit(sizes, n_sizes, log_blowup, log_last, n);
    if (rc != RSV_OK) return rc;
    if (!d_layers && sizes[0] - 1 - log_last - log_blowup > 0) return RSV_E_NULL;
    if (n_queries < 1 || n_queries > RSV_MAX_QUERIES || sub_log < 1 || sub_log > RSV_MAX_FRI_SUB_LOG) return RSV_E_SIZE;
    if (((uintptr_t)d_quot & 3) || ((uintptr_t)d_layers & 3) || ((uintptr_t)d_queries & 3) || ((uintptr_t)d_fri_witness & 3) ||
        ((uintptr_t)d_n_fri_witness & 3) || ((uintptr_t)d_hash_witness & 3) || ((uintptr_t)d_n_hash_witness & 3) || ((uintptr_t)d_caps & 3))
        return RSV_E_SIZE;
    return fri_open_cap(c, d_quot, d_layers, sizes, n_sizes, log_blowup, log_last, n, d_mask, d_queries, n_queries, d_fri_witness, d_n_fri_witness,
                        d_hash_witness, d_n_hash_witness, sub_log, d_caps);
}

}  // extern "C"
