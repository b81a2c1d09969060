// witness_api.inc — rsv_witness_program_* and rsv_witness_eval_dev (include/rsv.h): the recursion circuit's `variables`
// vector for a batch of proofs of one shape, evaluated level by level on the GPU (k_witness.hpp) from the hints of the
// verifying pass.  Included at the end of rsv_hip.hip.  The host-buffer forms stage through host_stage.inc (WitnessStage).

struct rsv_witness_program {
    int device = 0;
    uint32_t* d_instr = nullptr;
    uint32_t* d_levels = nullptr;       // level_offsets on the device (k_witness_strip)
    uint32_t strip_from = 0;            // first level of the narrow tail: every level from here on has <= STRIP_WIDTH instructions
    uint32_t walk_from = 0;             // first level of the medium tail: every level from here on has <= WALK_WIDTH instructions
    std::vector<uint32_t> level_offsets;
    uint32_t n_instr = 0, n_vars = 0;
    rsv_witness_shape shape{};
    std::vector<uint32_t> h_instr;      // rsv_witness_program_build keeps the host copy for rsv_witness_program_export
    std::vector<uint32_t> flow_wires;   // [copies * flow_count][5]: PoseidonEntry::wire of r1..r4, SwapOption::addr
    std::vector<uint32_t> gates;        // [n_rows][6]: a_wire, b_wire, c_wire, op, poseidon_wire, enforce_c_m31 (the template's)
    std::vector<uint32_t> witness_ops;  // [n][3]: row, bit variable, constant — rows whose op follows the witness
    // The chain's device copies (program_upload, trace_api.inc), each uploaded by the first call that needs it, under
    // trace_mu.  rsv_witness_trace_dev and after: the padded a / b / c wires [3][2^trace_lp] and witness_ops.
    std::mutex trace_mu;
    uint32_t* d_trace_wires = nullptr;
    uint32_t* d_trace_ops = nullptr;
    uint32_t trace_lp = 0, trace_lq = 0;
    // rsv_witness_interaction_dev and rsv_witness_commit_dev: the 10 + 40 preprocessed columns, [10][2^trace_lp] then
    // [40][2^trace_lq] (rsv_trace_preprocessed's order): the relations' columns and tree 0
    uint32_t* d_trace_pre = nullptr;
    // rsv_witness_eval_groups_dev: the copy that allocated each variable [n_vars] (built programs only; circuit_program.hpp)
    std::vector<uint8_t> copy_of;
    uint8_t* d_copy_of = nullptr;
    // rsv_circuit_program_create (user_circuit_api.inc): a caller's circuit has no instructions (n_instr = 0), and the
    // witness entry points refuse it; num_input is the reference's (3 for a built program: the recursion circuit has no
    // public input).  rsv_circuit_check_dev / rsv_circuit_flow_dev / rsv_circuit_eval_dev: the row and flow tables
    // (user_circuit_host.hpp) — uc: as check() resolved them when the program was created, with the evaluation program's
    // bits and links where it has one; empty for a built program, whose tables uc_upload resolves.
    uint32_t num_input = 3;
    rsv::ucircuit::Tables uc;
    uint32_t* d_uc_rows = nullptr;
    uint32_t* d_uc_flow = nullptr;
    // rsv_circuit_program_create_eval (circuit_eval_api.inc): the evaluation program (circuit_eval_host.hpp; none where
    // level_offsets is empty) and its device copies, uploaded by the first rsv_circuit_eval_dev: the instructions, then
    // level_offsets | flow_level_offsets | flow_order in one array.
    rsv::ceval::Program ce;
    uint32_t* d_ce_instr = nullptr;
    uint32_t* d_ce_index = nullptr;
    // Per-proof public inputs (rsv_witness_program_build_inputs, rsv_witness_eval_inputs_dev).  input_slots: 1 + the largest
    // imm0 of a W_INPUT, 0 for a program without one (every program has it: rsv_witness_program_create).  A built program
    // also knows the records it was built for (inputs_known): the idx of the n_fixed shared ones and of the n_own own ones;
    // d_own_idx: the latter on the device, uploaded by the builder.
    uint32_t input_slots = 0;
    bool inputs_known = false;
    std::vector<uint32_t> fixed_idx, own_idx;
    uint32_t* d_own_idx = nullptr;
    // A hashed program (rsv_witness_program_build_inputs_hashed): stmt_flow = S = ceil(copies * n_own / 8) + 1, the invocations
    // of the statement hash, whose records follow the members' in the flow buffers ([rows][S] behind [members][flow_count]);
    // 0 for every other program.
    uint32_t stmt_flow = 0;
};

namespace {

using rsv::circuit::FIXED_PART_WORDS;  // the constant-shape prefix of a proof (layout.hpp)
using rsv::circuit::check_program;
constexpr uint32_t STRIP_WIDTH = 32;  // levels this narrow at the end of a program run in one launch (k_witness_strip)
constexpr uint32_t WALK_WIDTH = 1536; // levels at most this wide behind the program's wide head: one launch for all of them in mid-size batches (below)
constexpr size_t SMALL_BATCH = 4;     // at most this many proofs: the whole program in one launch of one workgroup (k_witness_small; measured: one proof 0.71 -> 0.33 ms, four 0.75 -> 0.62, sixteen in ONE workgroup would lose: 0.8 -> 1.27)
// up to SMALL_MAX proofs: still one launch, a workgroup per 4 proofs, all of them side by side — if the program is short
// enough (SMALL_ROUNDS rounds of a workgroup's 1 024 lanes).  tools/witness_small_sweep.py, whole call, ms: level10 shape
// (47 788 instructions: 187 rounds) 8 proofs 2.20 -> 2.10, 256: 2.71 -> 2.58, 1 024: 3.39 -> 3.21, 2 048: 4.52 -> 4.68;
// level1 shape (321 865 instructions: 1 257 rounds) 8 proofs 2.32 -> 3.63, 1 024: 11.8 -> 12.7: not taken.
constexpr size_t SMALL_MAX = 1024;
constexpr uint64_t SMALL_ROUNDS = 384;

// accept[p] &= "the program applies to proof p" (same statement sizes and shape as the template's)
__global__ void k_witness_gate(const ProofMeta* __restrict__ metas, uint32_t n, rsv_witness_shape s, uint8_t* __restrict__ accept) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const ProofMeta& m = metas[p];
    const bool same = m.reason == R_OK && m.lp == s.log_size_plonk && m.lq == s.log_size_poseidon && m.pow_bits == s.pow_bits &&
                      m.blowup == s.log_blowup && m.log_last == s.log_last && m.nq == s.n_queries && m.n_inner == s.n_inner;
    if (!same) accept[p] = 0;
}

// accept[g] = every member of group g verified and has the program's shape (members: k_witness_gate's verdicts, [n_groups][copies])
__global__ void k_witness_group_accept(const uint8_t* __restrict__ members, uint32_t n_groups, uint32_t copies, uint8_t* __restrict__ accept) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    uint8_t all = 1;
    for (uint32_t c = 0; c < copies; c++) all &= members[(size_t)g * copies + c] != 0;
    accept[g] = all;
}

// Per-proof public inputs: rec[p] = the n_fixed shared records (fixed, in HBM), then proof p's n_own own ones — the array
// the verifying pass takes; one lane per word.  The lanes of an own record's words also check the statement against what
// the circuit can hold: idx is the program's (own_idx, NULL for a program made from instructions: not checked), and the
// value is an M31 — words 1..3 zero, word 0 below P (the PublicInput row enforces M31).  bad[p] is set otherwise (zeroed by the caller).
__global__ __launch_bounds__(256) void k_witness_statement(const uint32_t* __restrict__ fixed, uint32_t n_fixed, const uint32_t* __restrict__ own,
                                                           uint32_t n_own, const uint32_t* __restrict__ own_idx, uint32_t n,
                                                           uint32_t* __restrict__ rec, uint8_t* __restrict__ bad) {
    const uint32_t n_pi = n_fixed + n_own;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * n_pi * PI_WORDS) return;
    const uint32_t w = (uint32_t)(i % PI_WORDS);
    const size_t kp = i / PI_WORDS;
    const uint32_t k = (uint32_t)(kp % n_pi), p = (uint32_t)(kp / n_pi);
    if (k < n_fixed) { rec[i] = fixed[(size_t)k * PI_WORDS + w]; return; }
    const uint32_t j = k - n_fixed;
    const uint32_t v = own[((size_t)p * n_own + j) * PI_WORDS + w];
    rec[i] = v;
    const bool good = w == 0 ? (!own_idx || v == own_idx[j]) : w == 1 ? v < P : v == 0;
    if (!good) bad[p] = 1;  // (every writer stores the same byte)
}
// ... and behind the verifying pass: a proof whose statement the circuit cannot hold is rejected, as bad statement data is
__global__ void k_witness_statement_verdict(const uint8_t* __restrict__ bad, uint32_t n, uint8_t* __restrict__ accept, uint8_t* __restrict__ reason) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || !bad[p]) return;
    accept[p] = 0;
    if (reason) reason[p] = (uint8_t)R_PARSE;
}

// The program over n proofs (or n groups: a.n = n), in the launch form the batch size and the context's options choose:
// the kernels of k_witness.hpp over the argument type A.
template <class A>
void witness_launch(rsv_ctx* c, const rsv_witness_program* prog, A a, size_t n) {
    hipStream_t st = c->stream;
    const size_t n_levels = prog->level_offsets.size() - 1;
    // One launch for the whole program (k_witness_small) while a workgroup's share stays short: 2^log_p2 proofs per
    // workgroup = n_instr * 2^log_p2 / 1024 rounds of its 1 024 lanes + a barrier per level, about a microsecond each,
    // against ~140 launches with a drain between them (~0.75 ms) for the level form.
    uint32_t log_p2 = 0;
    if (n <= SMALL_BATCH) while ((1u << log_p2) < n) log_p2++;
    else log_p2 = c->opt.witness_small_log ? (uint32_t)c->opt.witness_small_log - 1 : 2u;
    const bool small = c->opt.witness_small_max ? n <= (size_t)c->opt.witness_small_max - 1
                                                : n <= SMALL_MAX && (((uint64_t)prog->n_instr << log_p2) >> 10) <= SMALL_ROUNDS;
    if (small) {
        hipLaunchKernelGGL(k_witness_small<A>, dim3(grid_for(n, 1u << log_p2)), dim3(1024), 0, st, a, prog->d_levels, (uint32_t)n_levels, log_p2);
    } else {
    // Mid-size batches: the wide head of the program level by level, then EVERYTHING behind it in one launch, a 1 024-lane
    // workgroup per 2^walk_log proofs walking the remaining levels (most of them ~100 instructions wide: a launch each
    // would be half launch gap).  RSV_OPT_WITNESS_WALK_LOG: 0 auto, 1 off, else 1 + log2(proofs per workgroup).
    uint32_t walk_log = 0;
    bool walk = false;
    if (c->opt.witness_walk_log >= 2) { walk = true; walk_log = (uint32_t)c->opt.witness_walk_log - 1; }
    else if (c->opt.witness_walk_log == 0) {  // measured (tools/witness_small_sweep.py, level10 shape, whole call): 2 048 proofs 4.55 -> 4.29 ms
        walk = true;                            // with 8 per workgroup, 4 096: 6.90 -> 6.66 and 8 192: 12.57 -> 12.17 with 16, 16 384: 24.18 -> 23.50 with 32
        walk_log = n <= 2048 ? 3u : n <= 8192 ? 4u : 5u;
    }
    const size_t head_end = walk ? prog->walk_from : prog->strip_from;
    for (size_t l = 0; l < head_end; l++) {
        a.begin = prog->level_offsets[l];
        a.end = prog->level_offsets[l + 1];
        if (a.end == a.begin) continue;
        if (n >= 64) {  // an instruction per blockIdx.y (65 535 at most per launch), proofs along x in blocks of 64 .. 256 lanes
            const uint32_t block = n >= 256 ? 256u : (uint32_t)((n + 63) / 64 * 64), end = a.end;
            for (uint32_t b = a.begin; b < end; b += 65535u) {
                a.begin = b;
                a.end = end - b > 65535u ? b + 65535u : end;
                hipLaunchKernelGGL(k_witness_level_wide<A>, dim3(grid_for(n, block), a.end - a.begin), dim3(block), 0, st, a);
            }
            continue;
        }
        const size_t threads = (size_t)(a.end - a.begin) * n;
        hipLaunchKernelGGL(k_witness_level<A>, dim3(grid_for(threads, 256)), dim3(256), 0, st, a);
    }
    if (walk && prog->walk_from < n_levels)
        hipLaunchKernelGGL(k_witness_small<A>, dim3(grid_for(n, 1u << walk_log)), dim3(1024), 0, st, a, prog->d_levels + prog->walk_from,
                           (uint32_t)(n_levels - prog->walk_from), walk_log);
    else if (prog->strip_from < n_levels)
        hipLaunchKernelGGL(k_witness_strip<A>, dim3(grid_for(n, 64)), dim3(256), 0, st, a, prog->d_levels, prog->strip_from, (uint32_t)n_levels);
    }
}

// The program over `rows` vectors of `per` proofs each (1: a batch of proofs; the copies of a group), in the instantiation it
// needs: Plain without own records, Input with them (d_pi [rows * per][n_own]), Stmt for a hashed program.  `a` is filled but
// for the own records and the statement; stmt, swap_used: witness_statement's and witness_hints'.
template <class Plain, class Input, class Stmt>
void witness_run(rsv_ctx* c, const rsv_witness_program* prog, Stmt& a, size_t rows, size_t per, const rsv_public_input* d_pi, size_t n_own,
                 rsv_public_input* stmt, uint8_t* swap_used) {
    if (!n_own) return witness_launch(c, prog, static_cast<const Plain&>(a), rows);
    a.own = reinterpret_cast<const PubInput*>(d_pi); a.n_own = (uint32_t)n_own;
    if (!prog->stmt_flow) return witness_launch(c, prog, static_cast<const Input&>(a), rows);
    // A hashed program: the statement of every row (its per * n_own records, copy-major) and the records of its hash, behind
    // the members' (a malformed record is the member's R_PARSE: k_witness_statement checks what the digest kernel would flag)
    const size_t tail = rows * per * prog->shape.flow_count;
    uint4* flow_tail = const_cast<uint4*>(a.flow) + tail * 8;
    statement_digest_launch(c, d_pi, rows, (uint32_t)(per * n_own), stmt, nullptr, flow_tail, swap_used + tail);
    a.stmt = reinterpret_cast<const PubInput*>(stmt); a.flow_tail = flow_tail;
    a.member_flow = (uint32_t)(per * prog->shape.flow_count); a.stmt_flow = prog->stmt_flow;
    witness_launch(c, prog, a, rows);
}

// The host-buffer forms of the witness chain (rsv_witness_eval, _trace, _interaction, _commit) on a batch stage
// (host_stage.inc): open(), the form's program upload and its outputs registered on b.s, eval(), the form's _dev calls on
// vars / flow / swap / accept, finish(), which copies every registered output back.
struct WitnessStage {
    BatchStage b;
    const uint32_t* vars = nullptr;     // eval()'s outputs on the device
    const uint32_t* flow = nullptr;     // NULL unless eval() was given flow buffers
    const uint8_t* swap = nullptr;
    const uint8_t* accept = nullptr;
    rsv_ctx* c() const { return b.c(); }

    // batch_offsets [batch_n + 1] have to be monotonic; by_variable: RSV_OPT_WITNESS_LAYOUT = 2, which the chain's kernels
    // read as they are written (no transpose, no second copy of the variables), else the default
    int open(const uint64_t* batch_offsets, size_t batch_n, int device, bool by_variable) {
        int rc = b.rebase(batch_offsets, batch_n);
        if (rc == RSV_OK) rc = b.create(device);
        if (rc != RSV_OK) return rc;
        if (by_variable) b.c()->opt.witness_layout = 2;
        return RSV_OK;
    }

    // variables, flow_out, swap_out: host buffers the results are copied back to, or NULL — then keep_flow says whether the
    // flow records are kept on the device at all (the chain's next stage reads them).  own, n_own: every proof's own records
    // [n][n_own] (host), behind the n_pi shared ones (rsv_witness_eval_inputs)
    int eval(const rsv_witness_program* prog, const uint8_t* blob, const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi,
             bool keep_flow, uint32_t* variables = nullptr, uint32_t* flow_out = nullptr, uint8_t* swap_out = nullptr,
             const rsv_public_input* own = nullptr, size_t n_own = 0) {
        const size_t n = b.n, flow_records = n * ((size_t)prog->shape.flow_count + prog->stmt_flow);
        uint32_t* d_flow = nullptr;
        uint8_t* d_swap = nullptr;
        if (keep_flow) {
            d_flow = flow_out ? b.s.output<uint32_t>(flow_out, flow_records * 128, true) : b.s.scratch<uint32_t>(flow_records * 128, true);
            d_swap = swap_out ? b.s.output<uint8_t>(swap_out, flow_records, true) : b.s.scratch<uint8_t>(flow_records, true);
        }
        (void)b.upload(blob);  // (its status is b.s.rc, looked at below)
        const size_t var_bytes = n * (size_t)prog->n_vars * 16;
        uint32_t* d_vars = variables ? b.s.output<uint32_t>(variables, var_bytes) : b.s.scratch<uint32_t>(var_bytes);
        const rsv_public_input* d_own = n_own ? b.s.upload<rsv_public_input>(own, sizeof(rsv_public_input) * n * n_own) : nullptr;
        if (b.s.rc != RSV_OK) return b.s.rc;
        vars = d_vars;
        flow = d_flow;
        swap = d_swap;
        accept = b.d_accept;
        if (n_own)
            return rsv_witness_eval_inputs_dev(b.c(), prog, b.d_blob, b.d_offsets, n, cfg, pi, n_pi, d_own, n_own, d_vars, d_flow, d_swap,
                                               b.d_accept, b.d_reason);
        return rsv_witness_eval_dev(b.c(), prog, b.d_blob, b.d_offsets, n, cfg, pi, n_pi, d_vars, d_flow, d_swap, b.d_accept, b.d_reason);
    }

    // Waits for the context, then copies the registered outputs, accept and reason (may be NULL) back.
    int finish(uint8_t* h_accept, uint8_t* h_reason) { return b.finish(h_accept, h_reason); }
};

}  // namespace

// rsv_witness_program_create; stmt_flow: the builder's, for a hashed program (its W_FLOW loads from the tail are in range)
static int witness_program_create(const uint32_t* instr, size_t n_instr, const uint32_t* level_offsets, size_t n_levels, uint32_t n_vars,
                                  const rsv_witness_shape* shape, int device, uint32_t stmt_flow, rsv_witness_program** out);

extern "C" {

int rsv_witness_program_create(const uint32_t* instr, size_t n_instr, const uint32_t* level_offsets, size_t n_levels,
                               uint32_t n_vars, const rsv_witness_shape* shape, int device, rsv_witness_program** out) {
    return witness_program_create(instr, n_instr, level_offsets, n_levels, n_vars, shape, device, 0, out);
}

}  // extern "C"

static int witness_program_create(const uint32_t* instr, size_t n_instr, const uint32_t* level_offsets, size_t n_levels, uint32_t n_vars,
                                  const rsv_witness_shape* shape, int device, uint32_t stmt_flow, rsv_witness_program** out) {
    if (!instr || !level_offsets || !shape || !out) return RSV_E_NULL;
    if (n_instr == 0 || n_instr > (1u << 26)) return RSV_E_SIZE;
    int rc = check_program(instr, n_instr, level_offsets, n_levels, n_vars, *shape, g_debug_log.load() != 0, stmt_flow);
    if (rc != RSV_OK) return rc;
    rc = select_device(device);
    if (rc != RSV_OK) return rc;
    rsv_witness_program* p = new (std::nothrow) rsv_witness_program();
    if (!p) return RSV_E_DEVICE;
    p->device = device;
    p->n_instr = (uint32_t)n_instr;
    p->n_vars = n_vars;
    p->shape = *shape;
    p->stmt_flow = stmt_flow;
    p->level_offsets.assign(level_offsets, level_offsets + n_levels + 1);
    for (size_t k = 0; k < n_instr; k++)
        if (instr[k * 8] == W_INPUT && instr[k * 8 + 4] >= p->input_slots) p->input_slots = instr[k * 8 + 4] + 1;
    p->strip_from = (uint32_t)n_levels;
    while (p->strip_from > 0 && level_offsets[p->strip_from] - level_offsets[p->strip_from - 1] <= STRIP_WIDTH) p->strip_from--;
    if (n_levels - p->strip_from < 8) p->strip_from = (uint32_t)n_levels;  // not worth a launch of its own
    p->walk_from = (uint32_t)n_levels;
    while (p->walk_from > 0 && level_offsets[p->walk_from] - level_offsets[p->walk_from - 1] <= WALK_WIDTH) p->walk_from--;
    if (p->walk_from > p->strip_from) p->walk_from = p->strip_from;
    if (hipMalloc(reinterpret_cast<void**>(&p->d_instr), n_instr * 32) != hipSuccess ||
        hipMemcpy(p->d_instr, instr, n_instr * 32, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&p->d_levels), (n_levels + 1) * 4) != hipSuccess ||
        hipMemcpy(p->d_levels, level_offsets, (n_levels + 1) * 4, hipMemcpyHostToDevice) != hipSuccess) {
        rsv_witness_program_destroy(p);
        return RSV_E_DEVICE;
    }
    *out = p;
    return RSV_OK;
}

extern "C" {

void rsv_witness_program_destroy(rsv_witness_program* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->d_instr) (void)hipFree(p->d_instr);
    if (p->d_levels) (void)hipFree(p->d_levels);
    if (p->d_trace_wires) (void)hipFree(p->d_trace_wires);
    if (p->d_trace_ops) (void)hipFree(p->d_trace_ops);
    if (p->d_trace_pre) (void)hipFree(p->d_trace_pre);
    if (p->d_copy_of) (void)hipFree(p->d_copy_of);
    if (p->d_own_idx) (void)hipFree(p->d_own_idx);
    if (p->d_uc_rows) (void)hipFree(p->d_uc_rows);
    if (p->d_uc_flow) (void)hipFree(p->d_uc_flow);
    if (p->d_ce_instr) (void)hipFree(p->d_ce_instr);
    if (p->d_ce_index) (void)hipFree(p->d_ce_index);
    delete p;
}

// The context's scratch of one evaluation: the hints of `members` proofs and, with `with_vars`, vars[variable][row] of `rows`
// vectors (rows = members for a batch of proofs, the number of groups for groups).  base NULL: the size only.
struct WitnessScratch {
    uint32_t *trace_cols, *fri_cols;
    uint4* flow;
    uint8_t* flow_swap;
    uint4* vars;
    size_t bytes;
};
static WitnessScratch witness_carve(const rsv_witness_program* prog, char* base, size_t members, size_t rows, bool with_vars) {
    const rsv_witness_shape& s = prog->shape;
    const size_t nq = s.n_queries, nt = 1 + (size_t)s.n_inner;
    Carve cv{base};
    WitnessScratch w{};
    w.trace_cols = cv.take<uint32_t>(members * 4 * nq * 64);
    w.fri_cols = cv.take<uint32_t>(members * nt * nq * 24);
    w.flow = cv.take<uint4>((members * (size_t)s.flow_count + rows * (size_t)prog->stmt_flow) * 8);  // (a hashed program: the hash's records behind the members')
    w.flow_swap = cv.take<uint8_t>(members * (size_t)s.flow_count + rows * (size_t)prog->stmt_flow);
    if (with_vars) w.vars = cv.take<uint4>(rows * (size_t)prog->n_vars);
    w.bytes = cv.off + 4096;
    return w;
}

int rsv_witness_scratch_bytes(const rsv_witness_program* prog, size_t n, size_t* bytes) {
    if (!prog || !bytes) return RSV_E_NULL;
    if (prog->n_instr == 0) return RSV_E_SIZE;  // a caller's circuit: nothing evaluates its witness
    *bytes = witness_carve(prog, nullptr, n, n, true).bytes;  // under RSV_OPT_WITNESS_LAYOUT = 2 the variables are not held twice: n * n_vars * 16 less
    return RSV_OK;
}

int rsv_witness_group_scratch_bytes(const rsv_witness_program* prog, size_t n_groups, size_t* bytes) {
    if (!prog || !bytes) return RSV_E_NULL;
    if (prog->copy_of.empty()) return RSV_E_SIZE;  // built programs only
    *bytes = witness_carve(prog, nullptr, n_groups * (size_t)prog->shape.copies, n_groups, true).bytes;
    return RSV_OK;
}

// the program belongs to one configuration: the batch has to be verified under exactly that one
static int witness_check_cfg(const rsv_witness_program* prog, const rsv_cfg_set* cfg) {
    const rsv_witness_shape& s = prog->shape;
    if (!cfg || !cfg->cfgs || cfg->n_cfgs != 1 || cfg->cfg_of) return RSV_E_SIZE;
    const rsv_pcs_config& pc = cfg->cfgs[0];
    if (pc.pow_bits != s.pow_bits || pc.log_blowup_factor != s.log_blowup || pc.log_last_layer_degree_bound != s.log_last ||
        pc.n_queries != s.n_queries)
        return RSV_E_SIZE;
    return RSV_OK;
}

// What both forms of the evaluation do before the program runs: the configuration check, the scratch, the verifying pass
// over `members` proofs with the hint outputs the program reads, and the members' verdicts (d_verdict, d_reason: the pass's,
// then k_witness_gate).  Fills `a` for `rows` vectors, all but a.accept.  d_own_pi: NULL — `pi` is the batch's one table, in
// host memory; else [members][n_pi] records in HBM, every proof its own (rsv_verify_hints_inputs_dev).
static int witness_hints(rsv_ctx* c, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets, size_t members,
                         size_t rows, const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, const rsv_public_input* d_own_pi,
                         uint32_t* d_variables, uint32_t* d_flow, uint8_t* d_flow_swap, uint8_t* d_verdict, uint8_t* d_reason, WitnessArgs& a,
                         uint8_t** flow_swap_used = nullptr) {
    const rsv_witness_shape& s = prog->shape;
    int rc = witness_check_cfg(prog, cfg);
    if (rc != RSV_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const bool by_variable = c->opt.witness_layout == 2;  // the caller takes vars[variable][row] as the kernels write it
    rc = ensure_buf(c, &c->ws_witness, &c->ws_witness_bytes, witness_carve(prog, nullptr, members, rows, !by_variable).bytes);
    if (rc != RSV_OK) return rc;
    const size_t nq = s.n_queries, nt = 1 + (size_t)s.n_inner;
    const uint32_t M = (s.log_size_plonk + 1 > s.log_size_poseidon + 2 ? s.log_size_plonk + 1 : s.log_size_poseidon + 2) + s.log_blowup;
    WitnessScratch w = witness_carve(prog, static_cast<char*>(c->ws_witness), members, rows, !by_variable);
    if (d_flow) {  // the caller keeps the PoseidonFlow (the next prover needs it beside the variables): written there directly
        w.flow = reinterpret_cast<uint4*>(d_flow);
        w.flow_swap = d_flow_swap;
    }
    if (by_variable) w.vars = reinterpret_cast<uint4*>(d_variables);
    rsv_hints_out ho{};
    ho.n_queries = s.n_queries; ho.max_log = M; ho.n_inner = s.n_inner;
    // the column values only: the sibling hashes of the paths are single-use halves of the circuit (no variables; their
    // values are in the flow records), so the per-query sibling paths are not asked for
    ho.d_trace_cols = w.trace_cols;
    ho.d_fri_cols = w.fri_cols;
    ho.d_flow = reinterpret_cast<uint32_t*>(w.flow);
    ho.d_flow_swap = w.flow_swap;
    ho.flow_stride = s.flow_count;
    // a proof of another shape may be shorter than the program's columns: nothing of an earlier batch may be read for it
    HIP_TRY(hipMemsetAsync(w.trace_cols, 0, members * 4 * nq * 64 * 4, c->stream));
    HIP_TRY(hipMemsetAsync(w.fri_cols, 0, members * nt * nq * 24 * 4, c->stream));
    rc = d_own_pi ? rsv_verify_hints_inputs_dev(c, d_blob, d_offsets, members, cfg, d_own_pi, n_pi, &ho, d_verdict, d_reason)
                  : rsv_verify_hints_dev(c, d_blob, d_offsets, members, cfg, pi, n_pi, &ho, d_verdict, d_reason);
    if (rc != RSV_OK) return rc;
    hipLaunchKernelGGL(k_witness_gate, dim3(grid_for(members, 256)), dim3(256), 0, c->stream, c->last_metas, (uint32_t)members, s, d_verdict);
    a.instr = prog->d_instr; a.n = (uint32_t)rows; a.vars = w.vars; a.blob = d_blob; a.offsets = d_offsets; a.metas = c->last_metas;
    a.flow = w.flow; a.flow_stride = s.flow_count; a.trace_cols = w.trace_cols; a.fri_cols = w.fri_cols;
    a.nq = s.n_queries; a.n_trees = (uint32_t)nt;
    if (flow_swap_used) *flow_swap_used = w.flow_swap;
    return RSV_OK;
}

// vars[variable][row] -> d_variables[row][variable], unless the caller takes the kernels' layout (then vars IS d_variables)
static int witness_finish(rsv_ctx* c, const rsv_witness_program* prog, const uint4* vars, uint32_t* d_variables, size_t rows) {
    if (c->opt.witness_layout != 2)
        hipLaunchKernelGGL(k_witness_transpose, dim3(grid_for(prog->n_vars, 32), grid_for(rows, 32)), dim3(256), 0, c->stream, vars,
                           reinterpret_cast<uint4*>(d_variables), prog->n_vars, (uint32_t)rows);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

// What the per-proof forms refuse before any device work (include/rsv.h): members = the proofs of the batch.
static int witness_check_own(const rsv_witness_program* prog, const rsv_public_input* pi_fixed, size_t n_fixed, const rsv_public_input* d_pi,
                             size_t n_own, size_t members) {
    if ((n_fixed && !pi_fixed) || (n_own && !d_pi)) return RSV_E_NULL;
    if (n_fixed > 4096 || n_own > MAX_OWN_INPUTS || n_fixed + n_own > 4096) return RSV_E_SIZE;
    if (prog->inputs_known) {  // a built program: the records it was built for
        if (n_fixed != prog->fixed_idx.size() || n_own != prog->own_idx.size()) return RSV_E_SIZE;
        for (size_t k = 0; k < n_fixed; k++)
            if (pi_fixed[k].idx != prog->fixed_idx[k]) return RSV_E_SIZE;
    } else if (prog->input_slots > n_own) return RSV_E_SIZE;  // made from instructions: every W_INPUT's imm0 lies below n_own
    if ((uint64_t)members * (n_fixed + n_own) > RSV_MAX_INPUT_RECORDS) return RSV_E_SIZE;
    if ((uintptr_t)d_pi & 3) return RSV_E_SIZE;
    return RSV_OK;
}
// The per-proof _dev forms: that, and with own records what the verifying pass would refuse of the batch itself, ahead of the
// statement kernel, so that a refused call has enqueued nothing
static int witness_check_inputs(const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets, size_t members,
                                const rsv_cfg_set* cfg, const rsv_public_input* pi_fixed, size_t n_fixed, const rsv_public_input* d_pi,
                                size_t n_own) {
    int rc = witness_check_own(prog, pi_fixed, n_fixed, d_pi, n_own, members);
    if (rc != RSV_OK || !n_own) return rc;
    rc = witness_check_cfg(prog, cfg);
    if (rc != RSV_OK) return rc;
    if (members && (!d_blob || !d_offsets)) return RSV_E_NULL;
    if (((uintptr_t)d_blob & 3) || ((uintptr_t)d_offsets & 7)) return RSV_E_SIZE;
    return RSV_OK;
}

// What the four _dev forms of the evaluation refuse first.  Where they differ — d_variables' alignment ahead of or behind the
// empty batch, the batch limit ahead of or behind the records' checks — the check stands at the entry point.
static int witness_check_call(const rsv_ctx* c, const rsv_witness_program* prog, const uint32_t* d_variables, const uint32_t* d_flow,
                              const uint8_t* d_flow_swap, const uint8_t* d_accept) {
    if (!c || !prog || !d_variables || !d_accept) return RSV_E_NULL;
    if ((d_flow == nullptr) != (d_flow_swap == nullptr)) return RSV_E_NULL;
    if (((uintptr_t)d_flow & 15) || prog->n_instr == 0) return RSV_E_SIZE;  // (a caller's circuit has no instructions)
    return RSV_OK;
}

// The per-proof forms, ahead of the verifying pass: the record array it takes, [members][n_fixed + n_own], assembled in the
// context's scratch from the shared records (host) and the caller's own ones (HBM), and the statement check; no host
// synchronisation.  -> rec, bad [members] (k_witness_statement).
static int witness_statement(rsv_ctx* c, const rsv_witness_program* prog, const rsv_public_input* pi_fixed, size_t n_fixed,
                             const rsv_public_input* d_pi, size_t n_own, size_t members, const rsv_public_input** rec, const uint8_t** bad,
                             size_t stmt_rows = 0, rsv_public_input** stmt = nullptr) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t n_pi = n_fixed + n_own, words = members * n_pi * PI_WORDS;
    Carve sz{nullptr};
    sz.take<uint32_t>(words); sz.take<uint32_t>(n_fixed * PI_WORDS); sz.take<uint32_t>(stmt_rows * STMT_WORDS * PI_WORDS); sz.take<uint8_t>(members);
    int rc = ensure_buf(c, &c->ws_inputs, &c->ws_inputs_bytes, sz.off);
    if (rc != RSV_OK) return rc;
    Carve cv{static_cast<char*>(c->ws_inputs)};
    uint32_t* d_rec = cv.take<uint32_t>(words);
    uint32_t* d_fixed = cv.take<uint32_t>(n_fixed * PI_WORDS);
    uint32_t* d_stmt = cv.take<uint32_t>(stmt_rows * STMT_WORDS * PI_WORDS);  // a hashed program: the statement of every row (k_statement_digest)
    if (stmt) *stmt = reinterpret_cast<rsv_public_input*>(d_stmt);
    uint8_t* d_bad = cv.take<uint8_t>(members);
    if (n_fixed) HIP_TRY(hipMemcpyAsync(d_fixed, pi_fixed, sizeof(rsv_public_input) * n_fixed, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_bad, 0, members, c->stream));
    hipLaunchKernelGGL(k_witness_statement, dim3(grid_for(words, 256)), dim3(256), 0, c->stream, d_fixed, (uint32_t)n_fixed,
                       reinterpret_cast<const uint32_t*>(d_pi), (uint32_t)n_own, prog->d_own_idx, (uint32_t)members, d_rec, d_bad);
    *rec = reinterpret_cast<const rsv_public_input*>(d_rec);
    *bad = d_bad;
    return RSV_OK;
}

// rsv_witness_eval_dev (d_pi NULL, n_own 0: `pi` is the batch's table) and rsv_witness_eval_inputs_dev (`pi`: the n_pi shared
// records, d_pi [n][n_own]: every proof's own)
static int witness_eval_impl(rsv_ctx* c, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                             const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, const rsv_public_input* d_pi, size_t n_own,
                             uint32_t* d_variables, uint32_t* d_flow, uint8_t* d_flow_swap, uint8_t* d_accept, uint8_t* d_reason) {
    const rsv_public_input* rec = nullptr;
    const uint8_t* bad = nullptr;
    rsv_public_input* stmt = nullptr;
    uint8_t* swap_used = nullptr;
    const size_t S = prog->stmt_flow;
    int rc = n_own ? witness_statement(c, prog, pi, n_pi, d_pi, n_own, n, &rec, &bad, S ? n : 0, &stmt) : RSV_OK;
    if (rc != RSV_OK) return rc;
    WitnessStmtArgs a{};
    rc = witness_hints(c, prog, d_blob, d_offsets, n, n, cfg, pi, n_pi + n_own, rec, d_variables, d_flow, d_flow_swap, d_accept, d_reason, a, &swap_used);
    if (rc != RSV_OK) return rc;
    a.accept = d_accept;
    if (n_own)
        hipLaunchKernelGGL(k_witness_statement_verdict, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, bad, (uint32_t)n, d_accept, d_reason);
    witness_run<WitnessArgs, WitnessInputArgs>(c, prog, a, n, 1, d_pi, n_own, stmt, swap_used);
    return witness_finish(c, prog, a.vars, d_variables, n);
}

int rsv_witness_eval_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                         const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint32_t* d_variables, uint32_t* d_flow,
                         uint8_t* d_flow_swap, uint8_t* d_accept, uint8_t* d_reason) {
    const int rc = witness_check_call(c, prog, d_variables, d_flow, d_flow_swap, d_accept);
    if (rc != RSV_OK) return rc;
    if (prog->input_slots) return RSV_E_SIZE;  // a program with own inputs: rsv_witness_eval_inputs_dev
    if (n == 0) return RSV_OK;
    if (n > (1u << 20) || prog->device != c->device || ((uintptr_t)d_variables & 15)) return RSV_E_SIZE;
    return witness_eval_impl(c, prog, d_blob, d_offsets, n, cfg, pi, n_pi, nullptr, 0, d_variables, d_flow, d_flow_swap, d_accept, d_reason);
}

int rsv_witness_eval_inputs_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                                const rsv_cfg_set* cfg, const rsv_public_input* pi_fixed, size_t n_fixed, const rsv_public_input* d_pi,
                                size_t n_own, uint32_t* d_variables, uint32_t* d_flow, uint8_t* d_flow_swap, uint8_t* d_accept,
                                uint8_t* d_reason) {
    int rc = witness_check_call(c, prog, d_variables, d_flow, d_flow_swap, d_accept);
    if (rc != RSV_OK) return rc;
    if (prog->stmt_flow && prog->shape.copies != 1) return RSV_E_SIZE;  // a hashed program of several copies hashes a GROUP's statements
    rc = witness_check_inputs(prog, d_blob, d_offsets, n, cfg, pi_fixed, n_fixed, d_pi, n_own);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    if (n > (1u << 20) || prog->device != c->device || ((uintptr_t)d_variables & 15)) return RSV_E_SIZE;
    return witness_eval_impl(c, prog, d_blob, d_offsets, n, cfg, pi_fixed, n_fixed, n_own ? d_pi : nullptr, n_own, d_variables, d_flow,
                             d_flow_swap, d_accept, d_reason);
}

// rsv_witness_eval_groups_dev and rsv_witness_eval_groups_inputs_dev (d_pi [n_groups * copies][n_own]: every member's own)
static int witness_groups_impl(rsv_ctx* c, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n_groups,
                               const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, const rsv_public_input* d_pi, size_t n_own,
                               uint32_t* d_variables, uint32_t* d_flow, uint8_t* d_flow_swap, uint8_t* d_accept, uint8_t* d_member_accept,
                               uint8_t* d_member_reason) {
    const size_t copies = prog->shape.copies, members = n_groups * copies;
    const rsv_public_input* rec = nullptr;
    const uint8_t* bad = nullptr;
    rsv_public_input* stmt = nullptr;
    uint8_t* swap_used = nullptr;
    const size_t S = prog->stmt_flow;
    int rc = n_own ? witness_statement(c, prog, pi, n_pi, d_pi, n_own, members, &rec, &bad, S ? n_groups : 0, &stmt) : RSV_OK;
    if (rc != RSV_OK) return rc;
    WitnessGroupStmtArgs a{};  // d_flow is [n_groups][copies][flow_count]: the members' records, one proof after the other
    rc = witness_hints(c, prog, d_blob, d_offsets, members, n_groups, cfg, pi, n_pi + n_own, rec, d_variables, d_flow, d_flow_swap,
                       d_member_accept, d_member_reason, a, &swap_used);
    if (rc != RSV_OK) return rc;
    {   // the table of copies goes to the device on the first call
        rsv_witness_program* wp = const_cast<rsv_witness_program*>(prog);
        std::lock_guard<std::mutex> lk(wp->trace_mu);
        if (!wp->d_copy_of) {
            uint8_t* d = nullptr;
            if (hipMalloc(reinterpret_cast<void**>(&d), wp->copy_of.size()) != hipSuccess) return RSV_E_DEVICE;
            if (hipMemcpy(d, wp->copy_of.data(), wp->copy_of.size(), hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipFree(d);
                return RSV_E_DEVICE;
            }
            wp->d_copy_of = d;
        }
    }
    if (n_own)
        hipLaunchKernelGGL(k_witness_statement_verdict, dim3(grid_for(members, 256)), dim3(256), 0, c->stream, bad, (uint32_t)members,
                           d_member_accept, d_member_reason);
    hipLaunchKernelGGL(k_witness_group_accept, dim3(grid_for(n_groups, 256)), dim3(256), 0, c->stream, d_member_accept, (uint32_t)n_groups,
                       (uint32_t)copies, d_accept);
    a.accept = d_accept; a.copy_of = prog->d_copy_of; a.copies = (uint32_t)copies;
    witness_run<WitnessGroupArgs, WitnessGroupInputArgs>(c, prog, a, n_groups, copies, d_pi, n_own, stmt, swap_used);
    return witness_finish(c, prog, a.vars, d_variables, n_groups);
}

int rsv_witness_eval_groups_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n_groups,
                                const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint32_t* d_variables, uint32_t* d_flow,
                                uint8_t* d_flow_swap, uint8_t* d_accept, uint8_t* d_member_accept, uint8_t* d_member_reason) {
    if (!d_member_accept) return RSV_E_NULL;
    const int rc = witness_check_call(c, prog, d_variables, d_flow, d_flow_swap, d_accept);
    if (rc != RSV_OK) return rc;
    if (prog->copy_of.empty() || ((uintptr_t)d_variables & 15)) return RSV_E_SIZE;  // only a built program knows which copy a hint belongs to
    if (prog->input_slots) return RSV_E_SIZE;  // a program with own inputs: rsv_witness_eval_groups_inputs_dev
    if (n_groups == 0) return RSV_OK;
    if (n_groups > (1u << 20) / prog->shape.copies || prog->device != c->device) return RSV_E_SIZE;
    return witness_groups_impl(c, prog, d_blob, d_offsets, n_groups, cfg, pi, n_pi, nullptr, 0, d_variables, d_flow, d_flow_swap, d_accept,
                               d_member_accept, d_member_reason);
}

int rsv_witness_eval_groups_inputs_dev(rsv_ctx* c, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets,
                                       size_t n_groups, const rsv_cfg_set* cfg, const rsv_public_input* pi_fixed, size_t n_fixed,
                                       const rsv_public_input* d_pi, size_t n_own, uint32_t* d_variables, uint32_t* d_flow,
                                       uint8_t* d_flow_swap, uint8_t* d_accept, uint8_t* d_member_accept, uint8_t* d_member_reason) {
    if (!d_member_accept) return RSV_E_NULL;
    int rc = witness_check_call(c, prog, d_variables, d_flow, d_flow_swap, d_accept);
    if (rc != RSV_OK) return rc;
    if (prog->copy_of.empty() || ((uintptr_t)d_variables & 15)) return RSV_E_SIZE;
    if (n_groups > (1u << 20) / prog->shape.copies) return RSV_E_SIZE;  // (here ahead of the records' checks: the members are a product)
    rc = witness_check_inputs(prog, d_blob, d_offsets, n_groups * prog->shape.copies, cfg, pi_fixed, n_fixed, d_pi, n_own);
    if (rc != RSV_OK) return rc;
    if (n_groups == 0) return RSV_OK;
    if (prog->device != c->device) return RSV_E_SIZE;
    return witness_groups_impl(c, prog, d_blob, d_offsets, n_groups, cfg, pi_fixed, n_fixed, n_own ? d_pi : nullptr, n_own, d_variables, d_flow,
                               d_flow_swap, d_accept, d_member_accept, d_member_reason);
}

int rsv_witness_program_inputs(const rsv_witness_program* prog, uint32_t* n_fixed, uint32_t* n_own, uint32_t* idx) {
    if (!prog) return RSV_E_NULL;
    if (!prog->inputs_known) return RSV_E_SIZE;  // only a built program knows the records it was built for
    if (n_fixed) *n_fixed = (uint32_t)prog->fixed_idx.size();
    if (n_own) *n_own = (uint32_t)prog->own_idx.size();
    if (idx && !prog->own_idx.empty()) std::memcpy(idx, prog->own_idx.data(), prog->own_idx.size() * 4);
    return RSV_OK;
}

// What rsv_witness_eval (own NULL, n_own 0) and rsv_witness_eval_inputs do after their own checks: a stage of its own, and
// the variables and the flow records (the latter form's include a hashed program's statement hash) copied back
static int witness_eval_host(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                             const rsv_public_input* pi, size_t n_pi, const rsv_public_input* own, size_t n_own, uint32_t* variables,
                             uint32_t* flow, uint8_t* flow_swap, uint8_t* accept, uint8_t* reason, int device) {
    return nomem_guard([&]() -> int {
        WitnessStage st;
        int rc = st.open(offsets, n, device, false);
        if (rc == RSV_OK) rc = st.eval(prog, blob, cfg, pi, n_pi, flow != nullptr, variables, flow, flow_swap, own, n_own);
        return rc == RSV_OK ? st.finish(accept, reason) : rc;
    });
}

int rsv_witness_eval(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                     const rsv_public_input* pi, size_t n_pi, uint32_t* variables, uint32_t* flow, uint8_t* flow_swap, uint8_t* accept,
                     uint8_t* reason, int device) {
    if (!prog || (n && (!blob || !offsets || !variables || !accept))) return RSV_E_NULL;
    if ((flow == nullptr) != (flow_swap == nullptr)) return RSV_E_NULL;
    if (prog->n_instr == 0) return RSV_E_SIZE;  // a caller's circuit
    if (n == 0) return RSV_OK;
    if (n > (1u << 20)) return RSV_E_SIZE;
    return witness_eval_host(prog, blob, offsets, n, cfg, pi, n_pi, nullptr, 0, variables, flow, flow_swap, accept, reason, device);
}

// the same with every proof's own records [n][n_own] behind the n_fixed shared ones, all in host memory
int rsv_witness_eval_inputs(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                            const rsv_public_input* pi_fixed, size_t n_fixed, const rsv_public_input* pi_own, size_t n_own, uint32_t* variables,
                            uint32_t* flow, uint8_t* flow_swap, uint8_t* accept, uint8_t* reason, int device) {
    if (!prog || (n && (!blob || !offsets || !variables || !accept))) return RSV_E_NULL;
    if ((flow == nullptr) != (flow_swap == nullptr)) return RSV_E_NULL;
    if (prog->n_instr == 0) return RSV_E_SIZE;  // a caller's circuit
    if (n > (1u << 20)) return RSV_E_SIZE;
    const int rc = witness_check_own(prog, pi_fixed, n_fixed, pi_own, n_own, n);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    return witness_eval_host(prog, blob, offsets, n, cfg, pi_fixed, n_fixed, pi_own, n_own, variables, flow, flow_swap, accept, reason, device);
}

int rsv_witness_program_statement(const rsv_witness_program* prog, uint32_t* hashed, uint32_t* n_words, uint32_t* stmt_flow_count) {
    if (!prog) return RSV_E_NULL;
    if (hashed) *hashed = prog->stmt_flow != 0;
    if (n_words) *n_words = prog->stmt_flow ? STMT_WORDS : 0;
    if (stmt_flow_count) *stmt_flow_count = prog->stmt_flow;
    return RSV_OK;
}

}  // extern "C"
