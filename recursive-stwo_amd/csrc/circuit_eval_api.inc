// circuit_eval_api.inc — rsv_circuit_program_create_eval (a caller's circuit with an evaluation program: host work only,
// circuit_eval_host.hpp), rsv_circuit_eval_info / _export, and rsv_circuit_eval_dev (`variables`, the flow and the swap
// bytes of a batch of witnesses from their free inputs, k_circuit_eval.hpp); include/rsv.h.  Included at the end of
// rsv_hip.hip.

namespace {

// Batches up to this many witnesses walk the levels in one launch (k_ce_walk), larger ones take a launch per level
// (k_ce_level).  The walk gives a witness one workgroup: 256 lanes for a level's instructions, and a chain of dependent
// permutations costs it a barrier a link instead of a launch.  It stops paying where the batch alone fills the machine's
// lanes in the per-level form while a walking workgroup still runs a wide level in rounds of 256.  Measured
// (tools/bench_circuit_eval.py, the level10 recursion circuit as a created program: 373 levels, 40 224 instructions, 3 782
// invocations; whole call, ms, per level / walk): 1 witness 3.80 / 3.75, 16: 4.01 / 4.09, 64: 3.91 / 4.00, 256: 4.59 / 3.99,
// 1 024: 6.02 / 5.91, 4 096: 11.84 / 14.27.  Both are ~10 us a level until the batch fills the machine; a circuit with
// fewer instructions per level than this one only moves the crossover up.
constexpr size_t CE_WALK_MAX = 1024;

// The evaluation program's instructions and index, uploaded by the first call (under trace_mu); the flow table is
// uc_upload's.
int ce_upload(rsv_witness_program* prog) {
    std::lock_guard<std::mutex> lk(prog->trace_mu);
    if (prog->d_ce_instr) return RSV_OK;
    const rsv::ceval::Program& e = prog->ce;
    std::vector<uint32_t> index;
    try {
        index.insert(index.end(), e.level_offsets.begin(), e.level_offsets.end());
        index.insert(index.end(), e.flow_level_offsets.begin(), e.flow_level_offsets.end());
        index.insert(index.end(), e.flow_order.begin(), e.flow_order.end());
    } catch (const std::bad_alloc&) {
        return RSV_E_NOMEM;
    }
    uint32_t *di = nullptr, *dx = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&di), e.instr.size() * 4) != hipSuccess ||
        hipMemcpy(di, e.instr.data(), e.instr.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dx), index.size() * 4) != hipSuccess ||
        hipMemcpy(dx, index.data(), index.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        if (di) (void)hipFree(di);
        if (dx) (void)hipFree(dx);
        return RSV_E_DEVICE;
    }
    prog->d_ce_index = dx;
    prog->d_ce_instr = di;
    return RSV_OK;
}

}  // namespace

extern "C" {

int rsv_circuit_program_create_eval(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, const uint32_t* witness_ops,
                                    size_t n_witness_ops, uint32_t n_vars, uint32_t num_input, const uint32_t* hints, size_t n_hints,
                                    const uint32_t* flow_links, uint32_t n_inputs, int device, rsv_witness_program** out) {
    if (!out) return RSV_E_NULL;
    return nomem_guard([&]() -> int {
        rsv::ceval::Program e;
        const int rc = rsv::ceval::compile(gates, n_rows, flow_wires, n_flow, witness_ops, n_witness_ops, n_vars, num_input, hints, n_hints,
                                           flow_links, n_inputs, &e);
        if (rc != RSV_OK) return rc;
        rsv_witness_program* p = uc_new_program(gates, n_rows, flow_wires, n_flow, witness_ops, n_witness_ops, n_vars, num_input, device, std::move(e.tables));
        p->ce = std::move(e);
        *out = p;
        return RSV_OK;
    });
}

int rsv_circuit_eval_info(const rsv_witness_program* prog, uint32_t* n_inputs, uint32_t* n_levels, uint32_t* n_instr) {
    if (!prog) return RSV_E_NULL;
    if (prog->ce.level_offsets.empty()) return RSV_E_SIZE;
    if (n_inputs) *n_inputs = prog->ce.n_inputs;
    if (n_levels) *n_levels = (uint32_t)prog->ce.n_levels();
    if (n_instr) *n_instr = (uint32_t)(prog->ce.instr.size() / rsv::ceval::INSTR_WORDS);
    return RSV_OK;
}

int rsv_circuit_eval_export(const rsv_witness_program* prog, uint32_t* instr, uint32_t* level_offsets, uint32_t* flow_order,
                            uint32_t* flow_level_offsets) {
    if (!prog) return RSV_E_NULL;
    const rsv::ceval::Program& e = prog->ce;
    if (e.level_offsets.empty()) return RSV_E_SIZE;
    if (instr) std::copy(e.instr.begin(), e.instr.end(), instr);
    if (level_offsets) std::copy(e.level_offsets.begin(), e.level_offsets.end(), level_offsets);
    if (flow_order) std::copy(e.flow_order.begin(), e.flow_order.end(), flow_order);
    if (flow_level_offsets) std::copy(e.flow_level_offsets.begin(), e.flow_level_offsets.end(), flow_level_offsets);
    return RSV_OK;
}

int rsv_circuit_eval_scratch_bytes(const rsv_witness_program* prog, size_t n, size_t* bytes) {
    if (!prog || !bytes) return RSV_E_NULL;
    if (prog->ce.level_offsets.empty() || n > (1u << 20)) return RSV_E_SIZE;
    *bytes = 0;  // both forms write d_variables in the caller's layout as they go
    return RSV_OK;
}

int rsv_circuit_eval_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_inputs, size_t n, uint32_t* d_variables, uint32_t* d_flow,
                         uint8_t* d_flow_swap, uint8_t* d_ok, uint32_t* d_bad_input) {
    if (!c || !prog || !d_variables || !d_flow || !d_flow_swap || !d_ok || !d_bad_input) return RSV_E_NULL;
    const rsv::ceval::Program& e = prog->ce;
    if (e.level_offsets.empty()) return RSV_E_SIZE;
    if (!d_inputs && e.n_inputs) return RSV_E_NULL;
    if (((uintptr_t)d_inputs & 15) || ((uintptr_t)d_variables & 15) || ((uintptr_t)d_flow & 15) || ((uintptr_t)d_bad_input & 3)) return RSV_E_SIZE;
    if (prog->device != c->device || n > (1u << 20)) return RSV_E_SIZE;
    const size_t n_levels = e.n_levels();
    const bool walk = c->opt.circuit_eval_form ? c->opt.circuit_eval_form == 2 : n <= CE_WALK_MAX;
    if (!walk)
        for (size_t l = 0; l < n_levels; l++) {
            const uint64_t blocks = ((uint64_t)(e.level_offsets[l + 1] - e.level_offsets[l]) * n + 255) / 256 +
                                    ((uint64_t)(e.flow_level_offsets[l + 1] - e.flow_level_offsets[l]) * n + 255) / 256;
            if (blocks >= (1u << 31)) return RSV_E_SIZE;
        }
    const uint64_t input_blocks = ((uint64_t)e.n_inputs * n + 255) / 256;
    if (input_blocks >= (1u << 31)) return RSV_E_SIZE;
    if (n == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = uc_upload(const_cast<rsv_witness_program*>(prog));
    if (rc == RSV_OK) rc = ce_upload(const_cast<rsv_witness_program*>(prog));
    if (rc != RSV_OK) return rc;
    rsv::CeArgs a{};
    a.instr = reinterpret_cast<const uint4*>(prog->d_ce_instr);
    a.levels = prog->d_ce_index;
    a.flevels = prog->d_ce_index + (n_levels + 1);
    a.forder = prog->d_ce_index + 2 * (n_levels + 1);
    a.src = reinterpret_cast<const uint4*>(prog->d_uc_flow);
    a.n_levels = (uint32_t)n_levels;
    a.n_flow = (uint32_t)e.flow_order.size();
    a.n_vars = prog->n_vars;
    a.n_inputs = e.n_inputs;
    a.n = (uint32_t)n;
    a.by_variable = c->opt.witness_layout == 2;
    a.inputs = reinterpret_cast<const uint4*>(d_inputs);
    a.vars = reinterpret_cast<uint4*>(d_variables);
    a.flow = reinterpret_cast<uint4*>(d_flow);
    a.swap = d_flow_swap;
    a.ok = d_ok;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemsetAsync(d_bad_input, 0xff, n * 4, st));
    if (input_blocks) hipLaunchKernelGGL(rsv::k_ce_inputs, dim3((unsigned)input_blocks), dim3(256), 0, st, a.inputs, a.n_inputs, a.n, d_ok, d_bad_input);
    if (walk) {
        hipLaunchKernelGGL(rsv::k_ce_walk, dim3((unsigned)n), dim3(256), 0, st, a);
    } else {
        for (size_t l = 0; l < n_levels; l++) {
            a.ibegin = e.level_offsets[l]; a.iend = e.level_offsets[l + 1];
            a.fbegin = e.flow_level_offsets[l]; a.fend = e.flow_level_offsets[l + 1];
            a.arith_blocks = (uint32_t)(((uint64_t)(a.iend - a.ibegin) * n + 255) / 256);
            const uint32_t blocks = a.arith_blocks + (uint32_t)(((uint64_t)(a.fend - a.fbegin) * n + 255) / 256);
            if (blocks) hipLaunchKernelGGL(rsv::k_ce_level, dim3(blocks), dim3(256), 0, st, a);
        }
    }
    // behind everything that reads ok: the witnesses with an input word at or above P
    hipLaunchKernelGGL(rsv::k_uc_verdict, dim3(grid_for(n, 256)), dim3(256), 0, st, d_bad_input, (uint32_t)n, d_ok);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

}  // extern "C"
