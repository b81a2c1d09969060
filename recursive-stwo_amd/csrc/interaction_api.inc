// interaction_api.inc — rsv_witness_interaction_dev / rsv_witness_interaction: the interaction (logup) columns of the
// recursion circuit, tree 2 of the next proof, and its two claimed sums (k_interaction.hpp, include/rsv.h).  Included at
// the end of rsv_hip.hip, after trace_api.inc.

namespace {

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

int rsv_witness_interaction_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                                const uint8_t* d_accept, const uint32_t* d_lookup, size_t n, uint32_t* d_int_plonk,
                                uint32_t* d_int_poseidon, uint32_t* d_sums, uint8_t* d_ok) {
    if (!c || !prog || !d_plonk || !d_poseidon || !d_accept || !d_lookup || !d_int_plonk || !d_int_poseidon || !d_sums) return RSV_E_NULL;
    if (((uintptr_t)d_plonk & 3) || ((uintptr_t)d_poseidon & 3) || ((uintptr_t)d_lookup & 3) || ((uintptr_t)d_int_plonk & 7) ||
        ((uintptr_t)d_int_poseidon & 7) || ((uintptr_t)d_sums & 3))
        return RSV_E_SIZE;
    int rc = chain_begin(c, prog, n, true);
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
    cp.pre = prog->d_trace_pre;
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
    cq.pre = prog->d_trace_pre + rsv::trace::PLONK_PRE_COLS * N;
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
    return nomem_guard([&]() -> int {
        if (!prog || (n && (!blob || !offsets || !lookup || !int_plonk || !int_poseidon || !sums || !accept))) return RSV_E_NULL;
        if (prog->gates.empty() || prog->n_instr == 0 || n > (1u << 20)) return RSV_E_SIZE;  // built programs only: the witness is evaluated
        if (n == 0) return RSV_OK;
        WitnessStage st;
        int rc = st.open(offsets, n, device, true);
        if (rc == RSV_OK) rc = program_upload(const_cast<rsv_witness_program*>(prog), true);
        if (rc != RSV_OK) return rc;
        const size_t N = (size_t)1 << prog->trace_lp, Q = (size_t)1 << prog->trace_lq;
        HostStage& s = st.b.s;
        uint32_t* dplonk = s.scratch<uint32_t>(n * rsv::PLONK_COLS_K * N * 4);
        uint32_t* dposeidon = s.scratch<uint32_t>(n * rsv::POSEIDON_COLS_K * Q * 4);
        const uint32_t* dlookup = s.upload<uint32_t>(lookup, n * 32);
        uint32_t* dip = s.output<uint32_t>(int_plonk, n * rsv::INT_COLS * N * 4);
        uint32_t* diq = s.output<uint32_t>(int_poseidon, n * rsv::INT_COLS * Q * 4);
        uint32_t* dsums = s.output<uint32_t>(sums, n * 32);
        uint8_t* dok = ok ? s.output<uint8_t>(ok, n) : s.scratch<uint8_t>(n);
        if (s.rc != RSV_OK) return s.rc;
        rc = st.eval(prog, blob, cfg, pi, n_pi, true);
        if (rc == RSV_OK) rc = rsv_witness_trace_dev(st.c(), prog, st.vars, st.flow, st.swap, st.accept, n, dplonk, dposeidon, nullptr);
        if (rc == RSV_OK) rc = rsv_witness_interaction_dev(st.c(), prog, dplonk, dposeidon, st.accept, dlookup, n, dip, diq, dsums, dok);
        return rc == RSV_OK ? st.finish(accept, reason) : rc;
    });
}

}  // extern "C"
