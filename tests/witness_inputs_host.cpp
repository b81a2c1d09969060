// witness_inputs_host.cpp — TEST INFRASTRUCTURE: circuit_program.hpp's builder with a proof's OWN public inputs
// (rsv_witness_program_build_inputs), host only: g++, no HIP, no device; built twice by tests/test_witness_inputs_host.py,
// plainly and with -fsanitize=address,undefined, and run on its own.
//
//   witness_inputs_host program <hints file> <n_fixed> <out file>
//       parse_template + build_program with records [n_fixed, n_pi) of the hints file as own inputs, check_program on the
//       result, the layout of the input variables, and with n_fixed == n_pi the arrays of the earlier argument list; the
//       program is written out for comparison with the oracle's circuit.
//   witness_inputs_host refusals
//       check_program: W_INPUT with imm0 >= 4096; check_copies: a hint that lies in another copy's range, an input variable
//       out of its place.
//
// The hints file is tests/host_logic_asan.cpp's.  The out file: 8 header words (magic, n_vars, n_levels, flow wire words,
// gate words, witness-op words, num_input, 0), instr, level_offsets, flow_wires, gates, witness_ops, copy_of (a word each).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../recursive-stwo_amd/csrc/circuit_program.hpp"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

using namespace rsv;

static std::vector<uint32_t> read_words(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f);
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    CHECK(n > 0 && n % 4 == 0);
    std::vector<uint32_t> w((size_t)n / 4);
    CHECK(fread(w.data(), 4, w.size(), f) == w.size());
    fclose(f);
    return w;
}

static int run_program(const char* in_path, size_t n_fixed, const char* out_path) {
    const std::vector<uint32_t> file = read_words(in_path);
    CHECK(file.size() > 16 && file[0] == 0x52535648u);
    const size_t len = file[1], nq = file[2], M = file[3], n_inner = file[4], flow_count = file[5], n_pi = file[6], copies = file[7];
    const size_t nt = 1 + n_inner;
    CHECK(n_fixed <= n_pi);
    const uint32_t n_own = (uint32_t)(n_pi - n_fixed);
    size_t at = 16;
    auto take = [&](size_t words) { const uint32_t* p = file.data() + at; at += words; CHECK(at <= file.size()); return p; };
    const uint32_t* proof_w = take((len + 3) / 4);
    const uint32_t* trace_sib = take(4 * nq * M * 8);
    const uint32_t* trace_pos = take(4 * nq);
    const uint32_t* trace_cols = take(4 * nq * 64);
    const uint32_t* fri_sib = take(nt * nq * M * 8);
    const uint32_t* fri_cols = take(nt * nq * 24);
    const uint32_t* flow = take(flow_count * 32);
    const uint8_t* swap = reinterpret_cast<const uint8_t*>(take((flow_count + 3) / 4));
    const uint32_t* pi = take(n_pi * 5);
    const uint8_t* walks = reinterpret_cast<const uint8_t*>(take((copies + 3) / 4));
    CHECK(at == file.size());
    // exact-size heap copies, so that the sanitizer sees every read past an array's end
    std::vector<uint32_t> v_tsib(trace_sib, trace_sib + 4 * nq * M * 8), v_tpos(trace_pos, trace_pos + 4 * nq),
        v_tcols(trace_cols, trace_cols + 4 * nq * 64), v_fsib(fri_sib, fri_sib + nt * nq * M * 8), v_fcols(fri_cols, fri_cols + nt * nq * 24),
        v_flow(flow, flow + flow_count * 32), v_proof(proof_w, proof_w + (len + 3) / 4);
    std::vector<uint8_t> v_swap(swap, swap + flow_count), v_walks(walks, walks + copies);

    circuit::Template d{};
    CHECK(circuit::parse_template(reinterpret_cast<const uint8_t*>(v_proof.data()), len, d) == RSV_OK);
    d.trace_sib = v_tsib.data(); d.trace_pos = v_tpos.data(); d.trace_cols = v_tcols.data();
    d.fri_sib = v_fsib.data(); d.fri_cols = v_fcols.data();
    std::vector<std::pair<uint32_t, circuit::Q4>> inputs;
    for (size_t i = 0; i < n_pi; i++) inputs.push_back({pi[5 * i], circuit::Q4{pi[5 * i + 1], pi[5 * i + 2], pi[5 * i + 3], pi[5 * i + 4]}});
    circuit::BuiltProgram bp;
    CHECK(circuit::build_program(d, v_flow.data(), v_swap.data(), (uint32_t)flow_count, inputs, n_fixed, (uint32_t)copies, v_walks.data(), bp) == RSV_OK);
    CHECK(circuit::build_program(d, v_flow.data(), v_swap.data(), (uint32_t)flow_count, inputs, n_pi + 1, (uint32_t)copies, v_walks.data(), bp) == RSV_E_SIZE);

    // the input variables: 4 + c * n_own + k, the reference's PublicInput row each, before every copy
    CHECK(bp.num_input == 3 + copies * n_own && bp.copy_of.size() == bp.n_vars && bp.gates.size() >= 6 * (4 + copies * n_own));
    std::vector<uint32_t> seen(bp.n_vars, 0);
    size_t n_input_instr = 0;
    for (size_t i = 0; i < bp.n_vars; i++) {
        const uint32_t* in = &bp.instr[i * 8];
        CHECK(in[1] < bp.n_vars && !seen[in[1]]++);
        if (in[0] != W_INPUT) continue;
        n_input_instr++;
        const uint32_t v = in[1];
        CHECK(v >= 4 && v < 4 + copies * n_own && in[4] == (v - 4) % n_own && bp.copy_of[v] == (v - 4) / n_own);
        CHECK(i < bp.level_offsets[1]);  // level 0
        const uint32_t* row = &bp.gates[(size_t)v * 6];
        CHECK(row[0] == v && row[1] == 0 && row[2] == v && row[3] == 1 && row[4] == 0 && row[5] == 1);
    }
    CHECK(n_input_instr == copies * n_own);

    const size_t n_levels = bp.level_offsets.size() - 1;
    rsv_witness_shape shape{d.lp, d.lq, d.pow_bits, d.blowup, d.log_last, d.nq, d.n_inner, (uint32_t)flow_count, (uint32_t)copies};
    CHECK(circuit::check_program(bp.instr.data(), bp.n_vars, bp.level_offsets.data(), n_levels, (uint32_t)bp.n_vars, shape) == RSV_OK);
    for (size_t i = 0; i < bp.n_vars; i++)  // every W_INPUT pushed to the first imm0 out of range
        if (bp.instr[i * 8] == W_INPUT) {
            std::vector<uint32_t> bad(bp.instr);
            bad[i * 8 + 4] = MAX_OWN_INPUTS;
            CHECK(circuit::check_program(bad.data(), bp.n_vars, bp.level_offsets.data(), n_levels, (uint32_t)bp.n_vars, shape) == RSV_E_RANGE);
            bad[i * 8 + 4] = MAX_OWN_INPUTS - 1;
            CHECK(circuit::check_program(bad.data(), bp.n_vars, bp.level_offsets.data(), n_levels, (uint32_t)bp.n_vars, shape) == RSV_OK);
        }

    if (n_own == 0) {  // every record a constant: the arrays of the argument list without n_fixed
        circuit::BuiltProgram old;
        CHECK(circuit::build_program(d, v_flow.data(), v_swap.data(), (uint32_t)flow_count, inputs, (uint32_t)copies, v_walks.data(), old) == RSV_OK);
        CHECK(old.n_vars == bp.n_vars && old.instr == bp.instr && old.level_offsets == bp.level_offsets && old.flow_wires == bp.flow_wires &&
              old.gates == bp.gates && old.witness_ops == bp.witness_ops && old.copy_of == bp.copy_of && old.num_input == 3);
    }

    FILE* f = fopen(out_path, "wb");
    CHECK(f);
    const uint32_t hdr[8] = {0x52535651u, (uint32_t)bp.n_vars, (uint32_t)n_levels, (uint32_t)bp.flow_wires.size(), (uint32_t)bp.gates.size(),
                             (uint32_t)bp.witness_ops.size(), bp.num_input, 0};
    fwrite(hdr, 4, 8, f);
    fwrite(bp.instr.data(), 4, bp.instr.size(), f);
    fwrite(bp.level_offsets.data(), 4, bp.level_offsets.size(), f);
    fwrite(bp.flow_wires.data(), 4, bp.flow_wires.size(), f);
    fwrite(bp.gates.data(), 4, bp.gates.size(), f);
    fwrite(bp.witness_ops.data(), 4, bp.witness_ops.size(), f);
    const std::vector<uint32_t> copy_words(bp.copy_of.begin(), bp.copy_of.end());
    fwrite(copy_words.data(), 4, copy_words.size(), f);
    fclose(f);
    printf("program: %zu variables, %zu levels, %zu rows, num_input %u\n", bp.n_vars, n_levels, bp.gates.size() / 6, bp.num_input);
    return 0;
}

static int run_refusals() {
    // check_program (what rsv_witness_program_create runs): a two-instruction program, an input and a copy of it
    const rsv_witness_shape shape{4, 8, 0, 1, 0, 4, 1, 16, 1};
    const uint32_t levels[3] = {0, 1, 2};
    auto program = [](uint32_t imm0) {
        return std::vector<uint32_t>{W_INPUT, 0, 0, 0, imm0, 0, 0, 0, W_COPY, 1, 0, 0, 0, 0, 0, 0};
    };
    for (uint32_t k : {0u, 1u, MAX_OWN_INPUTS - 1}) CHECK(circuit::check_program(program(k).data(), 2, levels, 2, 2, shape) == RSV_OK);
    for (uint32_t k : {MAX_OWN_INPUTS, MAX_OWN_INPUTS + 1, 0x7FFFFFFFu, 0xFFFFFFFFu})
        CHECK(circuit::check_program(program(k).data(), 2, levels, 2, 2, shape) == RSV_E_RANGE);
    {
        std::vector<uint32_t> beyond = program(0);
        beyond[0] = W_N_OPS;  // the op behind W_INPUT is none
        CHECK(circuit::check_program(beyond.data(), 2, levels, 2, 2, shape) == RSV_E_RANGE);
    }

    // check_copies: two copies with one own input each — variables 4 and 5 — and one hint each, variables 6 and 7
    using circuit::Instr;
    using circuit::mk_instr;
    std::vector<Instr> origin;
    for (uint32_t k = 0; k < 4; k++) origin.push_back(mk_instr(W_CONST));
    origin.push_back(mk_instr(W_INPUT, 0, 0, 0));
    origin.push_back(mk_instr(W_INPUT, 0, 0, 0));
    origin.push_back(mk_instr(W_WORD, 0, 0, 2));
    origin.push_back(mk_instr(W_WORD, 0, 0, 2));
    for (uint32_t k = 0; k < origin.size(); k++) origin[k].dst = k;
    const std::vector<uint8_t> copy_of{0, 0, 0, 0, 0, 1, 0, 1};
    const std::vector<uint32_t> marks{6, 7, 8};
    CHECK(circuit::check_copies(origin, copy_of, marks, 2, 1) == RSV_OK);
    {
        std::vector<uint8_t> c2(copy_of);
        c2[6] = 1;  // copy 1's hint inside copy 0's range
        CHECK(circuit::check_copies(origin, c2, marks, 2, 1) == RSV_E_RANGE);
        c2 = copy_of;
        c2[7] = 0;
        CHECK(circuit::check_copies(origin, c2, marks, 2, 1) == RSV_E_RANGE);
        c2 = copy_of;
        c2[7] = 2;  // a copy that does not exist
        CHECK(circuit::check_copies(origin, c2, marks, 2, 1) == RSV_E_RANGE);
        c2 = copy_of;
        c2[5] = 0;  // copy 1's input given to copy 0
        CHECK(circuit::check_copies(origin, c2, marks, 2, 1) == RSV_E_RANGE);
    }
    {
        std::vector<uint32_t> m2{6, 8, 8};  // the hint of copy 1 falls into copy 0's range: a hint range crossing copies
        CHECK(circuit::check_copies(origin, copy_of, m2, 2, 1) == RSV_E_RANGE);
        m2 = {5, 7, 8};  // the copies start inside the inputs
        CHECK(circuit::check_copies(origin, copy_of, m2, 2, 1) == RSV_E_RANGE);
        m2 = {6, 7};
        CHECK(circuit::check_copies(origin, copy_of, m2, 2, 1) == RSV_E_RANGE);
        m2 = {6, 7, 9};
        CHECK(circuit::check_copies(origin, copy_of, m2, 2, 1) == RSV_E_RANGE);
    }
    {
        std::vector<Instr> o2(origin);
        o2[4].imm[0] = 1;  // record 1 of one
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1) == RSV_E_RANGE);
        o2 = origin;
        o2[7] = mk_instr(W_INPUT, 0, 0, 0);  // an input behind the first copy's start
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1) == RSV_E_RANGE);
        o2 = origin;
        o2[5] = mk_instr(W_WORD, 0, 0, 2);  // something else in an input's place
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1) == RSV_E_RANGE);
        CHECK(circuit::check_copies(origin, copy_of, marks, 2, 2) == RSV_E_RANGE);  // two own inputs per copy: four variables
        CHECK(circuit::check_copies(origin, copy_of, marks, 2, 4096) == RSV_E_RANGE);  // more inputs than variables
    }
    // without own inputs: the two hints in their copies' ranges, which begin at variable 4
    {
        std::vector<Instr> o3(origin.begin(), origin.begin() + 4);
        o3.push_back(mk_instr(W_WORD, 0, 0, 2));
        o3.push_back(mk_instr(W_WORD, 0, 0, 2));
        CHECK(circuit::check_copies(o3, {0, 0, 0, 0, 0, 1}, {4, 5, 6}, 2, 0) == RSV_OK);
        CHECK(circuit::check_copies(o3, {0, 0, 0, 0, 1, 1}, {4, 5, 6}, 2, 0) == RSV_E_RANGE);
    }
    printf("refusals: ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && std::string(argv[1]) == "program") return run_program(argv[2], (size_t)atol(argv[3]), argv[4]);
    if (argc == 2 && std::string(argv[1]) == "refusals") return run_refusals();
    fprintf(stderr, "usage: witness_inputs_host program <hints> <n_fixed> <out> | refusals\n");
    return 2;
}
