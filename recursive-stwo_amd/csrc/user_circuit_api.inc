// user_circuit_api.inc — rsv_circuit_program_create (a caller's own Plonk-with-Poseidon circuit as the chain's program:
// host work only, user_circuit_host.hpp) and rsv_circuit_check_dev / rsv_circuit_flow_dev (the reference's two pre-prove
// checks and the PoseidonFlow for a batch of witnesses in HBM, k_user_circuit.hpp); include/rsv.h.  Included at the end of
// rsv_hip.hip.

namespace {

// The row and flow tables, uploaded by the first call that reads them (under trace_mu): a built program has none yet.
int uc_upload(rsv_witness_program* prog) {
    std::lock_guard<std::mutex> lk(prog->trace_mu);
    if (prog->d_uc_rows) return RSV_OK;
    rsv::ucircuit::Tables& t = prog->uc;
    if (t.rows.empty()) {
        const int rc = nomem_guard([&] {
            return rsv::ucircuit::check(prog->gates.data(), prog->gates.size() / 6, prog->flow_wires.data(), prog->flow_wires.size() / 5,
                                        prog->witness_ops.data(), prog->witness_ops.size() / 3, prog->n_vars, prog->num_input, &t);
        });
        if (rc != RSV_OK) return rc;
    }
    uint32_t *dr = nullptr, *df = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&dr), t.rows.size() * 4) != hipSuccess) return RSV_E_DEVICE;
    if (hipMemcpy(dr, t.rows.data(), t.rows.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&df), t.flow.size() * 4) != hipSuccess ||
        hipMemcpy(df, t.flow.data(), t.flow.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dr);
        if (df) (void)hipFree(df);
        return RSV_E_DEVICE;
    }
    prog->d_uc_flow = df;
    prog->d_uc_rows = dr;
    return RSV_OK;
}

// What both calls share: the argument checks, the device copies, bad = all ones.
int uc_begin(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_variables, size_t n, uint8_t* d_ok, uint32_t* d_bad,
             rsv::UcArgs& a) {
    if (!c || !prog || !d_variables || !d_ok || !d_bad) return RSV_E_NULL;
    if (((uintptr_t)d_variables & 15) || ((uintptr_t)d_bad & 3)) return RSV_E_SIZE;
    int rc = chain_begin(c, prog, n, false);
    if (rc == RSV_OK) rc = uc_upload(const_cast<rsv_witness_program*>(prog));
    if (rc != RSV_OK || n == 0) return rc;
    a.vars = reinterpret_cast<const uint4*>(d_variables);
    a.n_vars = prog->n_vars;
    a.n = (uint32_t)n;
    a.by_variable = c->opt.witness_layout == 2;
    a.ok = d_ok;
    a.bad = d_bad;
    a.wires = prog->d_trace_wires;
    a.log_plonk = prog->trace_lp;
    a.rows = reinterpret_cast<const uint4*>(prog->d_uc_rows);
    a.n_rows = (uint32_t)(prog->gates.size() / 6);
    a.src = reinterpret_cast<const uint4*>(prog->d_uc_flow);
    a.n_flow = (uint32_t)(prog->flow_wires.size() / 5);
    HIP_TRY(hipMemsetAsync(d_bad, 0xff, n * 4, c->stream));
    return RSV_OK;
}

// The program of arrays that check() has passed, with the tables it resolved.  Throws std::bad_alloc.
rsv_witness_program* uc_new_program(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, const uint32_t* witness_ops,
                                    size_t n_witness_ops, uint32_t n_vars, uint32_t num_input, int device, rsv::ucircuit::Tables&& tables) {
    std::unique_ptr<rsv_witness_program> p(new rsv_witness_program());
    p->device = device;
    p->n_vars = n_vars;
    p->num_input = num_input;
    p->shape.flow_count = (uint32_t)n_flow;
    p->shape.copies = 1;
    p->level_offsets.assign(1, 0);  // no instructions, no levels
    p->gates.assign(gates, gates + n_rows * 6);
    p->flow_wires.assign(flow_wires, flow_wires + n_flow * 5);
    if (n_witness_ops) p->witness_ops.assign(witness_ops, witness_ops + n_witness_ops * 3);
    p->uc = std::move(tables);
    return p.release();
}

}  // namespace

extern "C" {

int rsv_circuit_program_create(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, const uint32_t* witness_ops,
                               size_t n_witness_ops, uint32_t n_vars, uint32_t num_input, int device, rsv_witness_program** out) {
    if (!out) return RSV_E_NULL;
    return nomem_guard([&]() -> int {
        rsv::ucircuit::Tables t;
        const int rc = rsv::ucircuit::check(gates, n_rows, flow_wires, n_flow, witness_ops, n_witness_ops, n_vars, num_input, &t);
        if (rc != RSV_OK) return rc;
        *out = uc_new_program(gates, n_rows, flow_wires, n_flow, witness_ops, n_witness_ops, n_vars, num_input, device, std::move(t));
        return RSV_OK;
    });
}

int rsv_circuit_check_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_variables, size_t n, uint8_t* d_ok,
                          uint32_t* d_bad_row) {
    rsv::UcArgs a{};
    const int rc = uc_begin(c, prog, d_variables, n, d_ok, d_bad_row, a);
    if (rc != RSV_OK || n == 0) return rc;
    const uint64_t blocks = (uint64_t)((a.n_rows + 255) / 256) * n;
    if (blocks >= (1u << 31)) return RSV_E_SIZE;
    hipLaunchKernelGGL(rsv::k_uc_gates, dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(rsv::k_uc_verdict, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, d_bad_row, (uint32_t)n, d_ok);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int rsv_circuit_flow_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_variables, size_t n, uint32_t* d_flow,
                         uint8_t* d_flow_swap, uint8_t* d_ok, uint32_t* d_bad_flow) {
    if (!d_flow || !d_flow_swap) return RSV_E_NULL;
    if ((uintptr_t)d_flow & 15) return RSV_E_SIZE;
    rsv::UcArgs a{};
    const int rc = uc_begin(c, prog, d_variables, n, d_ok, d_bad_flow, a);
    if (rc != RSV_OK || n == 0) return rc;
    a.flow = reinterpret_cast<uint4*>(d_flow);
    a.swap = d_flow_swap;
    const uint64_t blocks = (uint64_t)((a.n_flow + rsv::TRACE_WAVE - 1) / rsv::TRACE_WAVE) * n;
    if (blocks >= (1u << 31)) return RSV_E_SIZE;
    hipLaunchKernelGGL(rsv::k_uc_flow, dim3((unsigned)blocks), dim3(rsv::TRACE_WAVE), 0, c->stream, a);
    hipLaunchKernelGGL(rsv::k_uc_verdict, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, d_bad_flow, (uint32_t)n, d_ok);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int rsv_circuit_program_num_input(const rsv_witness_program* prog, uint32_t* num_input) {
    if (!prog || !num_input) return RSV_E_NULL;
    if (prog->gates.empty()) return RSV_E_SIZE;
    *num_input = prog->num_input;
    return RSV_OK;
}

int rsv_circuit_inputs_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_variables, size_t n, rsv_public_input* d_pi) {
    if (!c || !prog || !d_variables || !d_pi) return RSV_E_NULL;
    if (prog->gates.empty() || n > (1u << 20) || ((uintptr_t)d_variables & 15) || ((uintptr_t)d_pi & 3)) return RSV_E_SIZE;
    if (prog->device != c->device) return RSV_E_SIZE;
    if (n == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t words = n * prog->num_input * rsv::PI_WORDS;  // (num_input < n_vars <= 2^26, n <= 2^20)
    if ((words + 255) / 256 >= (1u << 31)) return RSV_E_SIZE;
    hipLaunchKernelGGL(rsv::k_circuit_inputs, dim3(grid_for(words, 256)), dim3(256), 0, c->stream, d_variables, (uint32_t)n, prog->n_vars,
                       prog->num_input, c->opt.witness_layout == 2, reinterpret_cast<uint32_t*>(d_pi));
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

}  // extern "C"
