// trace_api.inc — rsv_trace_log_sizes / rsv_trace_preprocessed (host arithmetic, trace_host.hpp) and
// rsv_witness_trace_dev / rsv_witness_trace (the trace columns on the device, k_trace.hpp): the 110 columns the next
// prover commits for the recursion circuit of a batch (include/rsv.h).  Included at the end of rsv_hip.hip.

namespace {

// The program's device copies, each uploaded once (programs with a gate list only: RSV_E_SIZE otherwise): the padded wires and the
// witness ops, then, with `with_pre`, the 10 + 40 preprocessed columns that the interaction relations and tree 0 read.
int program_upload(rsv_witness_program* prog, bool with_pre) {
    std::lock_guard<std::mutex> lk(prog->trace_mu);
    if (!prog->d_trace_wires) {
        if (prog->gates.empty() || prog->flow_wires.empty()) return RSV_E_SIZE;
        const size_t n_rows = prog->gates.size() / 6;
        for (size_t i = 0; i < n_rows; i++)  // every index the kernels gather with
            for (int k = 0; k < 3; k++)
                if (prog->gates[i * 6 + k] >= prog->n_vars) return RSV_E_RANGE;
        for (size_t i = 0; i < prog->witness_ops.size() / 3; i++)
            if (prog->witness_ops[i * 3 + 1] >= prog->n_vars) return RSV_E_RANGE;
        uint32_t lp = 0, lq = 0;
        int rc = rsv::trace::log_sizes(n_rows, prog->flow_wires.size() / 5, lp, lq);
        if (rc != RSV_OK) return rc;
        const std::vector<uint32_t> wires = rsv::trace::padded_wires(prog->gates.data(), n_rows, lp);
        uint32_t *dw = nullptr, *dops = nullptr;
        const size_t ops_bytes = prog->witness_ops.size() * 4;
        if (hipMalloc(reinterpret_cast<void**>(&dw), wires.size() * 4) != hipSuccess) return RSV_E_DEVICE;
        if (hipMemcpy(dw, wires.data(), wires.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&dops), ops_bytes ? ops_bytes : 4) != hipSuccess ||
            (ops_bytes && hipMemcpy(dops, prog->witness_ops.data(), ops_bytes, hipMemcpyHostToDevice) != hipSuccess)) {
            (void)hipFree(dw);
            if (dops) (void)hipFree(dops);
            return RSV_E_DEVICE;
        }
        prog->d_trace_ops = dops;
        prog->trace_lp = lp;
        prog->trace_lq = lq;
        prog->d_trace_wires = dw;
    }
    if (!with_pre || prog->d_trace_pre) return RSV_OK;
    const uint32_t lp = prog->trace_lp, lq = prog->trace_lq;
    const size_t N = (size_t)1 << lp, Q = (size_t)1 << lq;
    std::vector<uint32_t> pre;
    int rc;
    try {
        pre.resize(rsv::trace::PLONK_PRE_COLS * N + rsv::trace::POSEIDON_PRE_COLS * Q);
        rc = rsv::trace::preprocessed(prog->gates.data(), prog->gates.size() / 6, prog->flow_wires.data(), prog->flow_wires.size() / 5, lp, lq,
                                      prog->num_input, rsv::RC_FULL_K, rsv::RC_PARTIAL_K, rsv::RC_FULL_K + 4, pre.data(),
                                      pre.data() + rsv::trace::PLONK_PRE_COLS * N);
    } catch (const std::bad_alloc&) {
        return RSV_E_NOMEM;
    }
    if (rc != RSV_OK) return rc;
    uint32_t* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), pre.size() * 4) != hipSuccess) return RSV_E_DEVICE;
    if (hipMemcpy(d, pre.data(), pre.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return RSV_E_DEVICE;
    }
    prog->d_trace_pre = d;
    return RSV_OK;
}

// What the chain's _dev forms do after their argument checks: the program's device and the batch limit, the context's
// device, the program's device copies (program_upload).
int chain_begin(rsv_ctx* c, const rsv_witness_program* prog, size_t n, bool with_pre) {
    if (prog->device != c->device || n > (1u << 20)) return RSV_E_SIZE;
    HIP_TRY(hipSetDevice(c->device));
    return program_upload(const_cast<rsv_witness_program*>(prog), with_pre);  // the lazily uploaded device copies only
}

}  // namespace

extern "C" {

int rsv_trace_log_sizes(size_t n_rows, size_t n_flow, uint32_t* log_plonk, uint32_t* log_poseidon) {
    if (!log_plonk || !log_poseidon) return RSV_E_NULL;
    return rsv::trace::log_sizes(n_rows, n_flow, *log_plonk, *log_poseidon);
}

int rsv_trace_preprocessed(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, uint32_t log_plonk,
                           uint32_t log_poseidon, uint32_t* plonk_pre, uint32_t* poseidon_pre) {
    return rsv_trace_preprocessed_inputs(gates, n_rows, flow_wires, n_flow, log_plonk, log_poseidon, rsv::trace::NUM_INPUT, plonk_pre,
                                         poseidon_pre);
}

int rsv_trace_preprocessed_inputs(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, uint32_t log_plonk,
                                  uint32_t log_poseidon, uint32_t num_input, uint32_t* plonk_pre, uint32_t* poseidon_pre) {
    return nomem_guard([&] {
        return rsv::trace::preprocessed(gates, n_rows, flow_wires, n_flow, log_plonk, log_poseidon, num_input, rsv::RC_FULL_K,
                                        rsv::RC_PARTIAL_K, rsv::RC_FULL_K + 4, plonk_pre, poseidon_pre);
    });
}

// rsv_witness_trace_dev (n proofs) and rsv_witness_trace_groups_dev (n groups, `grouped`): only the flow records differ
static int witness_trace(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_variables, const uint32_t* d_flow,
                         const uint8_t* d_flow_swap, const uint8_t* d_accept, size_t n, uint32_t* d_plonk, uint32_t* d_poseidon,
                         uint32_t* d_ops, bool grouped) {
    if (!c || !prog || !d_accept) return RSV_E_NULL;
    if ((d_plonk || d_ops) && !d_variables) return RSV_E_NULL;
    if (d_poseidon && (!d_flow || !d_flow_swap)) return RSV_E_NULL;
    if (((uintptr_t)d_variables & 15) || ((uintptr_t)d_flow & 15) || ((uintptr_t)d_poseidon & 15) || ((uintptr_t)d_plonk & 3) ||
        ((uintptr_t)d_ops & 3))
        return RSV_E_SIZE;
    int rc = chain_begin(c, prog, n, false);
    if (rc != RSV_OK) return rc;
    if (grouped && (prog->copy_of.empty() || n > (1u << 20) / prog->shape.copies)) return RSV_E_SIZE;  // built programs only (they have at least one copy)
    if (n == 0) return RSV_OK;
    const rsv_witness_shape& s = prog->shape;
    rsv::TraceStmtArgs a{};  // (the kernels of a program that is not hashed take its TraceArgs part)
    a.vars = reinterpret_cast<const uint4*>(d_variables);
    a.n_vars = prog->n_vars;
    a.n = (uint32_t)n;
    a.by_variable = c->opt.witness_layout == 2;
    a.accept = d_accept;
    a.wires = prog->d_trace_wires;
    a.log_plonk = prog->trace_lp;
    a.plonk = d_plonk;
    a.flow = reinterpret_cast<const uint4*>(d_flow);
    a.swap = d_flow_swap;
    a.flow_count = s.flow_count;
    a.copies = s.copies;
    a.n_pad = (uint32_t)rsv::trace::padded_flow((uint64_t)s.flow_count * s.copies + prog->stmt_flow);
    a.stmt_flow = prog->stmt_flow;
    a.tail = n * (size_t)s.flow_count * (grouped ? s.copies : 1u);  // the hash's records follow the members' (witness_api.inc)
    a.log_poseidon = prog->trace_lq;
    a.poseidon = d_poseidon;
    const uint64_t plonk_blocks = (uint64_t)((((size_t)1 << a.log_plonk) + 255) / 256) * n;
    const uint64_t poseidon_blocks = (uint64_t)((a.n_pad + rsv::TRACE_WAVE - 1) / rsv::TRACE_WAVE) * n;
    const size_t Q = (size_t)1 << a.log_poseidon, tail_first = (size_t)6 * a.n_pad;
    const uint64_t tail_threads = (uint64_t)(Q - tail_first) / 4 * rsv::POSEIDON_COLS_K * n;
    const size_t n_ops = prog->witness_ops.size() / 3;
    if (plonk_blocks >= (1u << 31) || poseidon_blocks >= (1u << 31) || tail_threads / 256 >= (1u << 31) || (uint64_t)n_ops * n / 256 >= (1u << 31))
        return RSV_E_SIZE;
    hipStream_t st = c->stream;
    const rsv::TraceArgs& plain = a;
    if (d_plonk) hipLaunchKernelGGL(rsv::k_trace_plonk, dim3((unsigned)plonk_blocks), dim3(256), 0, st, plain);
    if (d_ops && n_ops) hipLaunchKernelGGL(rsv::k_trace_ops, dim3(grid_for(n_ops * n, 256)), dim3(256), 0, st, plain, prog->d_trace_ops, (uint32_t)n_ops, d_ops);
    if (d_poseidon) {
        const auto launch = [&](const auto& args) {  // k_trace_poseidon<grouped, the argument type>
            using A = std::decay_t<decltype(args)>;
            hipLaunchKernelGGL((grouped ? rsv::k_trace_poseidon<true, A> : rsv::k_trace_poseidon<false, A>), dim3((unsigned)poseidon_blocks), dim3(rsv::TRACE_WAVE), 0, st, args);
        };
        if (prog->stmt_flow) launch(a);
        else launch(plain);
        if (tail_threads)
            hipLaunchKernelGGL(rsv::k_trace_zero_tail, dim3(grid_for(tail_threads, 256)), dim3(256), 0, st, d_poseidon, a.log_poseidon,
                               (uint32_t)tail_first, (uint64_t)rsv::POSEIDON_COLS_K * n);
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int rsv_witness_trace_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_variables, const uint32_t* d_flow,
                          const uint8_t* d_flow_swap, const uint8_t* d_accept, size_t n, uint32_t* d_plonk, uint32_t* d_poseidon,
                          uint32_t* d_ops) {
    return witness_trace(c, prog, d_variables, d_flow, d_flow_swap, d_accept, n, d_plonk, d_poseidon, d_ops, false);
}

int rsv_witness_trace_groups_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_variables, const uint32_t* d_flow,
                                 const uint8_t* d_flow_swap, const uint8_t* d_accept, size_t n_groups, uint32_t* d_plonk,
                                 uint32_t* d_poseidon, uint32_t* d_ops) {
    return witness_trace(c, prog, d_variables, d_flow, d_flow_swap, d_accept, n_groups, d_plonk, d_poseidon, d_ops, true);
}

int rsv_witness_trace(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                      const rsv_public_input* pi, size_t n_pi, uint32_t* plonk, uint32_t* poseidon, uint32_t* ops, uint8_t* accept,
                      uint8_t* reason, int device) {
    return nomem_guard([&]() -> int {
        if (!prog || (n && (!blob || !offsets || !accept))) return RSV_E_NULL;
        if (prog->gates.empty() || prog->n_instr == 0 || n > (1u << 20)) return RSV_E_SIZE;  // built programs only: the witness is evaluated
        if (n == 0) return RSV_OK;
        WitnessStage st;
        int rc = st.open(offsets, n, device, true);
        if (rc == RSV_OK) rc = program_upload(const_cast<rsv_witness_program*>(prog), false);
        if (rc != RSV_OK) return rc;
        const size_t N = (size_t)1 << prog->trace_lp, Q = (size_t)1 << prog->trace_lq, n_ops = prog->witness_ops.size() / 3;
        HostStage& s = st.b.s;
        uint32_t* dplonk = s.output<uint32_t>(plonk, n * rsv::PLONK_COLS_K * N * 4);
        uint32_t* dposeidon = s.output<uint32_t>(poseidon, n * rsv::POSEIDON_COLS_K * Q * 4);
        uint32_t* dops = s.output<uint32_t>(ops, n * n_ops * 4);
        if (s.rc != RSV_OK) return s.rc;
        rc = st.eval(prog, blob, cfg, pi, n_pi, true);
        if (rc == RSV_OK) rc = rsv_witness_trace_dev(st.c(), prog, st.vars, st.flow, st.swap, st.accept, n, dplonk, dposeidon, dops);
        return rc == RSV_OK ? st.finish(accept, reason) : rc;
    });
}

}  // extern "C"
