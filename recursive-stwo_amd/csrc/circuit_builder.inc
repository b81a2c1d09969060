// circuit_builder.inc — rsv_witness_program_build / _export (include/rsv.h): runs the mirrored gadgets (circuit_*.hpp) once
// over a template proof, with the hints of the GPU's own verifying pass, and turns what they did into a witness program.
// HOST code; included at the end of rsv_hip.hip behind witness_api.inc.  Everything that needs no device — locating the
// template's sections, replaying the gadgets, sorting the instructions into levels — is circuit_program.hpp.

using namespace rsv::circuit;

// The records of the statement hash of the TEMPLATE, for the builder of a hashed program: its own records `copies` times
// over (every copy of the template circuit verifies the template), hashed by the kernel the evaluation runs.
static int template_statement_flow(const rsv_public_input* own, size_t n_own, uint32_t copies, int device, std::vector<uint32_t>& flow) {
    return nomem_guard([&]() -> int {
        const size_t T = (size_t)copies * n_own, S = (T + 7) / 8 + 1;
        std::vector<rsv_public_input> rec;
        for (uint32_t c = 0; c < copies; c++) rec.insert(rec.end(), own, own + n_own);
        int rc = select_device(device);
        if (rc != RSV_OK) return rc;
        flow.resize(S * 32);
        BatchStage b;  // (no batch: the context of its own, and the teardown order)
        const rsv_public_input* d_rec = b.s.upload<rsv_public_input>(rec.data(), sizeof(rsv_public_input) * T);
        rsv_public_input* d_stmt = b.s.scratch<rsv_public_input>(sizeof(rsv_public_input) * STMT_WORDS);
        uint4* d_flow = b.s.output<uint4>(flow.data(), S * 128);
        uint8_t* d_swap = b.s.scratch<uint8_t>(S);
        if (b.s.rc != RSV_OK) return b.s.rc;
        rc = b.create(device);
        if (rc != RSV_OK) return rc;
        statement_digest_launch(b.c(), d_rec, 1, (uint32_t)T, d_stmt, nullptr, d_flow, d_swap);
        rc = hipGetLastError() == hipSuccess ? rsv_ctx_synchronize(b.c()) : RSV_E_DEVICE;
        return rc == RSV_OK ? b.s.finish() : rc;
    });
}

static int witness_program_build(const uint8_t* proof, size_t len, const rsv_pcs_config* cfg, const rsv_public_input* pi, size_t n_pi, size_t n_fixed,
                                 uint32_t copies, const uint8_t* set_walks, int device, bool hashed, rsv_witness_program** out);

extern "C" {

int rsv_witness_program_build_inputs(const uint8_t* proof, size_t len, const rsv_pcs_config* cfg, const rsv_public_input* pi, size_t n_pi,
                                     size_t n_fixed, uint32_t copies, const uint8_t* set_walks, int device, rsv_witness_program** out) {
    return witness_program_build(proof, len, cfg, pi, n_pi, n_fixed, copies, set_walks, device, false, out);
}

int rsv_witness_program_build_inputs_hashed(const uint8_t* proof, size_t len, const rsv_pcs_config* cfg, const rsv_public_input* pi, size_t n_pi,
                                            size_t n_fixed, uint32_t copies, const uint8_t* set_walks, int device, rsv_witness_program** out) {
    return witness_program_build(proof, len, cfg, pi, n_pi, n_fixed, copies, set_walks, device, true, out);
}

int rsv_witness_program_build(const uint8_t* proof, size_t len, const rsv_pcs_config* cfg, const rsv_public_input* pi, size_t n_pi,
                              uint32_t copies, const uint8_t* set_walks, int device, rsv_witness_program** out) {
    return rsv_witness_program_build_inputs(proof, len, cfg, pi, n_pi, n_pi, copies, set_walks, device, out);
}

}  // extern "C"

static int witness_program_build(const uint8_t* proof, size_t len, const rsv_pcs_config* cfg, const rsv_public_input* pi, size_t n_pi, size_t n_fixed,
                                 uint32_t copies, const uint8_t* set_walks, int device, bool hashed, rsv_witness_program** out) {
    if (!proof || !cfg || !out || (n_pi && !pi)) return RSV_E_NULL;
    if (copies == 0 || copies > 64 || n_fixed > n_pi || n_pi - n_fixed > MAX_OWN_INPUTS) return RSV_E_SIZE;
    if (hashed && n_fixed == n_pi) return RSV_E_SIZE;  // a hashed statement is the hash of own records
    Template d{};
    int rc = parse_template(proof, len, d);
    if (rc != RSV_OK) return rc;
    if (cfg->pow_bits != d.pow_bits || cfg->log_blowup_factor != d.blowup || cfg->log_last_layer_degree_bound != d.log_last ||
        cfg->n_queries != d.nq)
        return RSV_E_SIZE;
    uint32_t flow_count = 0;
    rc = rsv_poseidon_flow_count(d.lp, d.lq, cfg, &flow_count);
    if (rc != RSV_OK) return rc;
    // the template's hints from the GPU's own verifying pass
    const size_t nq = d.nq, M = d.M, nt = 1 + (size_t)d.n_inner;
    std::vector<uint32_t> trace_sib(4 * nq * M * 8), trace_pos(4 * nq), trace_cols(4 * nq * 64), fri_sib(nt * nq * M * 8), fri_cols(nt * nq * 24),
        flow((size_t)flow_count * 32);
    std::vector<uint8_t> swap(flow_count);
    rsv_hints_out ho{};
    ho.n_queries = d.nq; ho.max_log = d.M; ho.n_inner = d.n_inner;
    ho.d_trace_sib = trace_sib.data(); ho.d_trace_pos = trace_pos.data(); ho.d_trace_cols = trace_cols.data();
    ho.d_fri_sib = fri_sib.data(); ho.d_fri_cols = fri_cols.data();
    ho.d_flow = flow.data(); ho.d_flow_swap = swap.data(); ho.flow_stride = flow_count;
    const uint64_t offsets[2] = {0, len};
    const rsv_cfg_set cfg_set{cfg, 1, nullptr};
    uint8_t accept = 0, reason = 0;
    rc = rsv_verify_hints(proof, offsets, 1, &cfg_set, pi, n_pi, &ho, &accept, &reason, device);
    if (rc != RSV_OK) return rc;
    if (!accept) return RSV_E_RANGE;  // a template has to be a proof that verifies
    d.trace_sib = trace_sib.data(); d.trace_pos = trace_pos.data(); d.trace_cols = trace_cols.data();
    d.fri_sib = fri_sib.data(); d.fri_cols = fri_cols.data();

    std::vector<std::pair<uint32_t, Q4>> inputs;
    for (size_t i = 0; i < n_pi; i++) inputs.push_back({pi[i].idx, Q4{pi[i].value[0], pi[i].value[1], pi[i].value[2], pi[i].value[3]}});
    BuiltProgram bp;
    std::vector<uint32_t> stmt_flow;
    if (hashed) {
        for (size_t i = n_fixed; i < n_pi; i++)  // the circuit holds a hashed statement in M31 variables
            if (pi[i].value[0] >= P || pi[i].value[1] || pi[i].value[2] || pi[i].value[3]) return RSV_E_RANGE;
        rc = template_statement_flow(pi + n_fixed, n_pi - n_fixed, copies, device, stmt_flow);
        if (rc != RSV_OK) return rc;
    }
    rc = build_program(d, flow.data(), swap.data(), flow_count, inputs, n_fixed, copies, set_walks, bp, g_debug_log.load() != 0,
                       hashed ? stmt_flow.data() : nullptr, (uint32_t)(stmt_flow.size() / 32));
    if (rc != RSV_OK) return rc;
    rsv_witness_shape shape{d.lp, d.lq, d.pow_bits, d.blowup, d.log_last, d.nq, d.n_inner, flow_count, copies};
    rsv_witness_program* prog = nullptr;
    rc = witness_program_create(bp.instr.data(), bp.n_vars, bp.level_offsets.data(), bp.level_offsets.size() - 1, (uint32_t)bp.n_vars, &shape, device,
                                bp.stmt_flow_count, &prog);
    if (rc != RSV_OK) return rc;
    prog->h_instr = std::move(bp.instr);
    prog->flow_wires = std::move(bp.flow_wires);
    prog->gates = std::move(bp.gates);
    prog->witness_ops = std::move(bp.witness_ops);
    prog->copy_of = std::move(bp.copy_of);
    prog->num_input = bp.num_input;
    prog->inputs_known = true;
    for (size_t i = 0; i < n_pi; i++) (i < n_fixed ? prog->fixed_idx : prog->own_idx).push_back(pi[i].idx);
    if (!prog->own_idx.empty() &&  // the statement check's table (k_witness_statement)
        (hipMalloc(reinterpret_cast<void**>(&prog->d_own_idx), prog->own_idx.size() * 4) != hipSuccess ||
         hipMemcpy(prog->d_own_idx, prog->own_idx.data(), prog->own_idx.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) {
        rsv_witness_program_destroy(prog);
        return RSV_E_DEVICE;
    }
    *out = prog;
    return RSV_OK;
}

extern "C" {

int rsv_witness_program_gates(const rsv_witness_program* prog, uint32_t* n_rows, uint32_t* n_witness_ops, uint32_t* gates, uint32_t* witness_ops) {
    if (!prog) return RSV_E_NULL;
    if (prog->gates.empty()) return RSV_E_SIZE;  // only a built program knows the circuit's gate list
    if (n_rows) *n_rows = (uint32_t)(prog->gates.size() / 6);
    if (n_witness_ops) *n_witness_ops = (uint32_t)(prog->witness_ops.size() / 3);
    if (gates) std::memcpy(gates, prog->gates.data(), prog->gates.size() * 4);
    if (witness_ops) std::memcpy(witness_ops, prog->witness_ops.data(), prog->witness_ops.size() * 4);
    return RSV_OK;
}

int rsv_witness_program_info(const rsv_witness_program* prog, uint32_t* n_vars, uint32_t* n_levels, rsv_witness_shape* shape) {
    if (!prog) return RSV_E_NULL;
    if (n_vars) *n_vars = prog->n_vars;
    if (n_levels) *n_levels = (uint32_t)prog->level_offsets.size() - 1;
    if (shape) *shape = prog->shape;
    return RSV_OK;
}

int rsv_witness_program_export(const rsv_witness_program* prog, uint32_t* instr, uint32_t* level_offsets, uint32_t* flow_wires) {
    if (!prog) return RSV_E_NULL;
    if (instr && prog->n_instr) {
        if (prog->h_instr.empty()) {  // created from the caller's arrays: the copy lives on the device
            if (select_device(prog->device) != RSV_OK) return RSV_E_DEVICE;
            HIP_TRY(hipMemcpy(instr, prog->d_instr, (size_t)prog->n_instr * 32, hipMemcpyDeviceToHost));
        } else std::memcpy(instr, prog->h_instr.data(), prog->h_instr.size() * 4);
    }
    if (level_offsets) std::memcpy(level_offsets, prog->level_offsets.data(), prog->level_offsets.size() * 4);
    if (flow_wires) {
        if (prog->flow_wires.empty()) return RSV_E_SIZE;  // only a built program knows its flow's wires
        std::memcpy(flow_wires, prog->flow_wires.data(), prog->flow_wires.size() * 4);
    }
    return RSV_OK;
}

}  // extern "C"
