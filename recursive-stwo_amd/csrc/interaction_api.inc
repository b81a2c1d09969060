// interaction_api.inc — rsv_witness_interaction_dev / rsv_witness_interaction: the interaction (logup) columns of the
// recursion circuit, tree 2 of the next proof, and its two claimed sums (k_interaction.hpp, include/rsv.h).  Included at
// the end of rsv_hip.hip, after trace_api.inc.

namespace {

// The preprocessed columns the relations read, [8][2^lp] then [8][2^lq] on the device, uploaded once (after
// trace_upload, which checks the program and sets lp, lq).
int interaction_upload(rsv_witness_program* prog) {
    int rc = trace_upload(prog);
    if (rc != RSV_OK) return rc;
    std::lock_guard<std::mutex> lk(prog->trace_mu);
    if (prog->d_int_pre) return RSV_OK;
    const uint32_t lp = prog->trace_lp, lq = prog->trace_lq;
    const size_t N = (size_t)1 << lp, Q = (size_t)1 << lq;
    std::vector<uint32_t> plonk, poseidon, compact;
    try {
        plonk.resize(rsv::trace::PLONK_PRE_COLS * N);
        poseidon.resize(rsv::trace::POSEIDON_PRE_COLS * Q);
        compact.resize(rsv::INT_PRE_COLS * (N + Q));
    } catch (const std::bad_alloc&) {
        return RSV_E_NOMEM;
    }
    rc = rsv::trace::preprocessed(prog->gates.data(), prog->gates.size() / 6, prog->flow_wires.data(), prog->flow_wires.size() / 5, lp, lq,
                                  rsv::RC_FULL_K, rsv::RC_PARTIAL_K, rsv::RC_FULL_K + 4, plonk.data(), poseidon.data());
    if (rc != RSV_OK) return rc;
    // Plonk: a_wire, b_wire, c_wire, mult_a, mult_b, mult_c, poseidon_wire, mult_poseidon (op and enforce_c_m31 are read
    // by no relation); Poseidon: is_first, is_last, round_id, rc0[0], external_idx_1 / _2, their nonzero flags.
    static const uint32_t PC[8] = {0, 1, 2, 4, 5, 6, 7, 8}, QC[8] = {0, 1, 3, 4, 36, 37, 38, 39};
    for (int k = 0; k < 8; k++) {
        std::memcpy(compact.data() + k * N, plonk.data() + PC[k] * N, N * 4);
        std::memcpy(compact.data() + 8 * N + k * Q, poseidon.data() + QC[k] * Q, Q * 4);
    }
    uint32_t* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), compact.size() * 4) != hipSuccess) return RSV_E_DEVICE;
    if (hipMemcpy(d, compact.data(), compact.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return RSV_E_DEVICE;
    }
    prog->d_int_pre = d;
    return RSV_OK;
}

// Chunk bits of a component of 2^log rows for a batch of n: 2^(B-1) scan lanes per (proof, component), aiming at about
// 2^17 in all (2 components x n proofs x 2^(B-1)) but at least 64 and at most 2^(INT_MAX_B - 1) = 2 048 per proof, so a
// batch of fewer than 32 proofs has fewer (4 096 for one proof; the k_int_offsets scan of 2^B sums stays one workgroup);
// B <= log - 1.
uint32_t interaction_chunk_bits(uint32_t log, size_t n) {
    uint32_t ln = 0;
    while (((size_t)1 << ln) < n) ln++;
    uint32_t b = 17 - std::min<uint32_t>(ln, 10);  // 2^(b-1) lanes per (proof, component)
    b = std::min<uint32_t>(std::max<uint32_t>(b, 7), rsv::INT_MAX_B);
    return std::min<uint32_t>(b, log - 1);
}

}  // namespace

extern "C" {

int rsv_witness_interaction_dev(rsv_ctx* c, const rsv_witness_program* cprog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                                const uint8_t* d_accept, const uint32_t* d_lookup, size_t n, uint32_t* d_int_plonk,
                                uint32_t* d_int_poseidon, uint32_t* d_sums, uint8_t* d_ok) {
    if (!c || !cprog || !d_plonk || !d_poseidon || !d_accept || !d_lookup || !d_int_plonk || !d_int_poseidon || !d_sums) return RSV_E_NULL;
    if (((uintptr_t)d_plonk & 3) || ((uintptr_t)d_poseidon & 3) || ((uintptr_t)d_lookup & 3) || ((uintptr_t)d_int_plonk & 7) ||
        ((uintptr_t)d_int_poseidon & 7) || ((uintptr_t)d_sums & 3))
        return RSV_E_SIZE;
    if (cprog->device != c->device || n > (1u << 20)) return RSV_E_SIZE;
    rsv_witness_program* prog = const_cast<rsv_witness_program*>(cprog);  // the lazily uploaded device copies only
    HIP_TRY(hipSetDevice(c->device));
    int rc = interaction_upload(prog);
    if (rc != RSV_OK) return rc;
    const uint32_t lp = prog->trace_lp, lq = prog->trace_lq;
    if (lp < 2 || lq < 2) return RSV_E_SIZE;  // one chunk bit at least
    if (n == 0) return RSV_OK;
    const size_t N = (size_t)1 << lp, Q = (size_t)1 << lq;
    const uint32_t Bp = interaction_chunk_bits(lp, n), Bq = interaction_chunk_bits(lq, n);
    const uint64_t frac_p = (uint64_t)((N + 255) / 256) * n, frac_q = (uint64_t)((Q + 255) / 256) * n;
    const uint64_t scan_p = (uint64_t)(((1u << (Bp - 1)) + 63) / 64) * n, scan_q = (uint64_t)(((1u << (Bq - 1)) + 63) / 64) * n;
    if (frac_p >= (1u << 31) || frac_q >= (1u << 31) || scan_p >= (1u << 31) || scan_q >= (1u << 31)) return RSV_E_SIZE;
    Carve sz{nullptr};
    sz.take<uint32_t>(n);
    sz.take<uint4>(3 * n);
    sz.take<uint4>(2 * n);
    sz.take<uint4>(n << Bp);
    sz.take<uint4>(n << Bp);
    sz.take<uint4>(n << Bq);
    sz.take<uint4>(n << Bq);
    rc = ensure_buf(c, &c->ws_interaction, &c->ws_interaction_bytes, sz.off);
    if (rc != RSV_OK) return rc;
    Carve cv{static_cast<char*>(c->ws_interaction)};
    rsv::IntArgs a{};
    a.accept = d_accept;
    a.lookup = d_lookup;
    a.n = (uint32_t)n;
    a.bad = cv.take<uint32_t>(n);
    a.lk = cv.take<uint4>(3 * n);
    a.ok = d_ok;
    uint4* shifts = cv.take<uint4>(2 * n);
    rsv::IntComp& cp = a.c[0];
    cp.pre = prog->d_int_pre;
    cp.trace = d_plonk;
    cp.n_trace = rsv::PLONK_COLS_K;
    cp.log = lp;
    cp.B = Bp;
    cp.out = d_int_plonk;
    cp.start = cv.take<uint4>(n << Bp);
    cp.end = cv.take<uint4>(n << Bp);
    cp.shift = shifts;
    cp.sums = d_sums;
    rsv::IntComp& cq = a.c[1];
    cq.pre = prog->d_int_pre + rsv::INT_PRE_COLS * N;
    cq.trace = d_poseidon;
    cq.n_trace = rsv::POSEIDON_COLS_K;
    cq.log = lq;
    cq.B = Bq;
    cq.out = d_int_poseidon;
    cq.start = cv.take<uint4>(n << Bq);
    cq.end = cv.take<uint4>(n << Bq);
    cq.shift = shifts + n;
    cq.sums = d_sums + 4;
    // one launch per phase, both components side by side (blockIdx.y); the smaller one's surplus blocks exit at once
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(rsv::k_int_prep, dim3(grid_for(n, 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rsv::k_int_frac, dim3((unsigned)std::max(frac_p, frac_q), 2), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rsv::k_int_chunks, dim3((unsigned)std::max(scan_p, scan_q), 2), dim3(64), 0, st, a);
    hipLaunchKernelGGL(rsv::k_int_offsets, dim3((unsigned)n, 2), dim3(rsv::INT_OFF_THREADS), 0, st, a);
    hipLaunchKernelGGL(rsv::k_int_scan, dim3((unsigned)std::max(scan_p, scan_q), 2), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int rsv_witness_interaction(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                            const rsv_public_input* pi, size_t n_pi, const uint32_t* lookup, uint32_t* int_plonk, uint32_t* int_poseidon,
                            uint32_t* sums, uint8_t* ok, uint8_t* accept, uint8_t* reason, int device) {
    if (!prog || (n && (!blob || !offsets || !lookup || !int_plonk || !int_poseidon || !sums || !accept))) return RSV_E_NULL;
    if (prog->gates.empty() || n > (1u << 20)) return RSV_E_SIZE;  // built programs only, as rsv_witness_interaction_dev
    if (n == 0) return RSV_OK;
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return RSV_E_SIZE;
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    rsv_ctx* c = nullptr;
    rc = rsv_ctx_create(device, &c);
    if (rc != RSV_OK) return rc;
    struct Guard { rsv_ctx* c; ~Guard() { rsv_ctx_destroy(c); } } guard{c};
    c->opt.witness_layout = 2;  // as rsv_witness_trace: no transpose, no second copy
    rc = interaction_upload(const_cast<rsv_witness_program*>(prog));
    if (rc != RSV_OK) return rc;
    const size_t N = (size_t)1 << prog->trace_lp, Q = (size_t)1 << prog->trace_lq;
    const uint64_t base = offsets[0], total = offsets[n] - base;
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
    DevBuf dblob, doffs, dvars, dacc, dreason, dflow, dswap, dplonk, dposeidon, dlookup, dip, diq, dsums, dok;
    const size_t flow_records = n * (size_t)prog->shape.flow_count;
    HIP_TRY(dflow.alloc(flow_records * 128));
    HIP_TRY(dswap.alloc(flow_records));
    HIP_TRY(dblob.alloc(total));
    HIP_TRY(doffs.alloc(8 * (n + 1)));
    HIP_TRY(dvars.alloc(n * (size_t)prog->n_vars * 16));
    HIP_TRY(dacc.alloc(n));
    HIP_TRY(dreason.alloc(n));
    HIP_TRY(dplonk.alloc(n * rsv::PLONK_COLS_K * N * 4));
    HIP_TRY(dposeidon.alloc(n * rsv::POSEIDON_COLS_K * Q * 4));
    HIP_TRY(dlookup.alloc(n * 32));
    HIP_TRY(dip.alloc(n * rsv::INT_COLS * N * 4));
    HIP_TRY(diq.alloc(n * rsv::INT_COLS * Q * 4));
    HIP_TRY(dsums.alloc(n * 32));
    HIP_TRY(dok.alloc(n));
    HIP_TRY(hipMemcpy(dblob.p, blob + base, total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(doffs.p, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dlookup.p, lookup, n * 32, hipMemcpyHostToDevice));
    rc = rsv_witness_eval_dev(c, prog, dblob.as<const uint8_t>(), doffs.as<const uint64_t>(), n, cfg, pi, n_pi, dvars.as<uint32_t>(),
                              dflow.as<uint32_t>(), dswap.as<uint8_t>(), dacc.as<uint8_t>(), dreason.as<uint8_t>());
    if (rc != RSV_OK) return rc;
    rc = rsv_witness_trace_dev(c, prog, dvars.as<const uint32_t>(), dflow.as<const uint32_t>(), dswap.as<const uint8_t>(),
                               dacc.as<const uint8_t>(), n, dplonk.as<uint32_t>(), dposeidon.as<uint32_t>(), nullptr);
    if (rc != RSV_OK) return rc;
    rc = rsv_witness_interaction_dev(c, prog, dplonk.as<const uint32_t>(), dposeidon.as<const uint32_t>(), dacc.as<const uint8_t>(),
                                     dlookup.as<const uint32_t>(), n, dip.as<uint32_t>(), diq.as<uint32_t>(), dsums.as<uint32_t>(),
                                     dok.as<uint8_t>());
    if (rc != RSV_OK) return rc;
    rc = rsv_ctx_synchronize(c);
    if (rc != RSV_OK) return rc;
    HIP_TRY(hipMemcpy(int_plonk, dip.p, n * rsv::INT_COLS * N * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(int_poseidon, diq.p, n * rsv::INT_COLS * Q * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sums, dsums.p, n * 32, hipMemcpyDeviceToHost));
    if (ok) HIP_TRY(hipMemcpy(ok, dok.p, n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(accept, dacc.p, n, hipMemcpyDeviceToHost));
    if (reason) HIP_TRY(hipMemcpy(reason, dreason.p, n, hipMemcpyDeviceToHost));
    return RSV_OK;
}

}  // extern "C"
