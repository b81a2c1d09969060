// statement_host.cpp — TEST INFRASTRUCTURE: circuit_program.hpp's builder of a HASHED program
// (rsv_witness_program_build_inputs_hashed), host only: g++, no HIP, no device; built twice by tests/test_statement_host.py,
// plainly and with -fsanitize=address,undefined, and run on its own.
//
//   statement_host program <hints file> <n_fixed> <statement flow file> <out file>
//       parse_template + build_program with records [n_fixed, n_pi) of the hints file as own inputs and the records of
//       the statement hash (S x 32 words: left, right, out), check_program on the result, the layout of the statement and
//       input variables; the program is written out for comparison with the oracle's circuit.
//   statement_host refusals
//       build_program: no own input, a wrong count of hash records, an own value that is no M31; check_program: W_STMT with
//       imm0 >= 8, W_FLOW in and beyond the tail; check_copies: the placement of a hashed program.
//
// The hints file is tests/host_logic_asan.cpp's, the out file tests/witness_inputs_host.cpp's with header word 7 = S.
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

static int run_program(const char* in_path, size_t n_fixed, const char* stmt_path, const char* out_path) {
    const std::vector<uint32_t> file = read_words(in_path);
    const std::vector<uint32_t> v_stmt = read_words(stmt_path);  // (exact size: the sanitizer sees a read past its end)
    CHECK(file.size() > 16 && file[0] == 0x52535648u);
    const size_t len = file[1], nq = file[2], M = file[3], n_inner = file[4], flow_count = file[5], n_pi = file[6], copies = file[7];
    const size_t nt = 1 + n_inner;
    CHECK(n_fixed < n_pi);
    const uint32_t n_own = (uint32_t)(n_pi - n_fixed), T = (uint32_t)copies * n_own, S = (T + 7) / 8 + 1;
    CHECK(v_stmt.size() == (size_t)S * 32);
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
    auto build = [&](const std::vector<std::pair<uint32_t, circuit::Q4>>& in, size_t fixed, const std::vector<uint32_t>& stmt, uint32_t count,
                     circuit::BuiltProgram& bp) {
        return circuit::build_program(d, v_flow.data(), v_swap.data(), (uint32_t)flow_count, in, fixed, (uint32_t)copies, v_walks.data(), bp, false,
                                      stmt.data(), count);
    };
    circuit::BuiltProgram bp, scrap;
    CHECK(build(inputs, n_fixed, v_stmt, S, bp) == RSV_OK);
    CHECK(build(inputs, n_pi, v_stmt, S, scrap) == RSV_E_SIZE);      // no own input
    CHECK(build(inputs, n_fixed, v_stmt, S + 1, scrap) == RSV_E_SIZE);  // not the hash's count of invocations
    CHECK(build(inputs, n_fixed, v_stmt, S - 1, scrap) == RSV_E_SIZE);
    for (int w = 0; w < 4; w++) {  // an own value that is no M31
        auto odd = inputs;
        odd[n_fixed].second[w] = w ? 1u : 0x7fffffffu;
        CHECK(build(odd, n_fixed, v_stmt, S, scrap) == RSV_E_RANGE);
    }
    {   // a record of the hash that is not the circuit's invocation: its input, the capacity it continues from
        std::vector<uint32_t> other(v_stmt);
        other[0] ^= 1u;
        CHECK(build(inputs, n_fixed, other, S, scrap) == RSV_E_RANGE);
        other = v_stmt;
        other[(size_t)(S - 1) * 32 + 8] ^= 1u;
        CHECK(build(inputs, n_fixed, other, S, scrap) == RSV_E_RANGE);
    }

    // the statement 4 .. 11 (W_STMT, a PublicInput row each), the own records 12 .. 12 + T (W_INPUT, a witness row each)
    CHECK(bp.num_input == 11 && bp.stmt_flow_count == S && bp.copy_of.size() == bp.n_vars && bp.gates.size() >= 6 * (12 + (size_t)T));
    std::vector<uint32_t> seen(bp.n_vars, 0);
    size_t n_input_instr = 0, n_stmt_instr = 0, n_tail = 0;
    for (size_t i = 0; i < bp.n_vars; i++) {
        const uint32_t* in = &bp.instr[i * 8];
        CHECK(in[1] < bp.n_vars && !seen[in[1]]++);
        const uint32_t v = in[1];
        if (in[0] == W_FLOW && in[4] >= copies * flow_count) {
            CHECK(in[4] < copies * flow_count + S);
            n_tail++;
        }
        if (in[0] != W_INPUT && in[0] != W_STMT) continue;
        CHECK(i < bp.level_offsets[1]);  // level 0
        const uint32_t* row = &bp.gates[(size_t)v * 6];
        CHECK(row[0] == v && row[1] == 0 && row[2] == v && row[3] == 1 && row[4] == 0 && row[5] == 1);
        if (in[0] == W_STMT) {
            n_stmt_instr++;
            CHECK(v >= 4 && v < 12 && in[4] == v - 4);
        } else {
            n_input_instr++;
            CHECK(v >= 12 && v < 12 + T && in[4] == (v - 12) % n_own && bp.copy_of[v] == (v - 12) / n_own);
        }
    }
    CHECK(n_input_instr == T && n_stmt_instr == 8);
    CHECK(n_tail == 2 * (size_t)S);  // every invocation of the hash keeps one half: two variables
    CHECK(bp.flow_wires.size() == 5 * (copies * flow_count + S));

    const size_t n_levels = bp.level_offsets.size() - 1;
    rsv_witness_shape shape{d.lp, d.lq, d.pow_bits, d.blowup, d.log_last, d.nq, d.n_inner, (uint32_t)flow_count, (uint32_t)copies};
    CHECK(circuit::check_program(bp.instr.data(), bp.n_vars, bp.level_offsets.data(), n_levels, (uint32_t)bp.n_vars, shape, false, S) == RSV_OK);
    // ... and without the tail declared its W_FLOW loads are out of range
    CHECK(circuit::check_program(bp.instr.data(), bp.n_vars, bp.level_offsets.data(), n_levels, (uint32_t)bp.n_vars, shape) == RSV_E_RANGE);
    CHECK(circuit::check_program(bp.instr.data(), bp.n_vars, bp.level_offsets.data(), n_levels, (uint32_t)bp.n_vars, shape, false, S - 1) == RSV_E_RANGE);

    FILE* f = fopen(out_path, "wb");
    CHECK(f);
    const uint32_t hdr[8] = {0x52535651u, (uint32_t)bp.n_vars, (uint32_t)n_levels, (uint32_t)bp.flow_wires.size(), (uint32_t)bp.gates.size(),
                             (uint32_t)bp.witness_ops.size(), bp.num_input, bp.stmt_flow_count};
    fwrite(hdr, 4, 8, f);
    fwrite(bp.instr.data(), 4, bp.instr.size(), f);
    fwrite(bp.level_offsets.data(), 4, bp.level_offsets.size(), f);
    fwrite(bp.flow_wires.data(), 4, bp.flow_wires.size(), f);
    fwrite(bp.gates.data(), 4, bp.gates.size(), f);
    fwrite(bp.witness_ops.data(), 4, bp.witness_ops.size(), f);
    const std::vector<uint32_t> copy_words(bp.copy_of.begin(), bp.copy_of.end());
    fwrite(copy_words.data(), 4, copy_words.size(), f);
    fclose(f);
    printf("program: %zu variables, %zu levels, %zu rows, num_input %u, %u hash invocations\n", bp.n_vars, n_levels, bp.gates.size() / 6,
           bp.num_input, bp.stmt_flow_count);
    return 0;
}

static int run_refusals() {
    // check_program: a statement word and a load from the tail (two copies of 16 records, a hash of 3)
    const rsv_witness_shape shape{4, 8, 0, 1, 0, 4, 1, 16, 2};
    const uint32_t levels[3] = {0, 1, 2};
    auto program = [](uint32_t op, uint32_t imm0, uint32_t imm1) {
        return std::vector<uint32_t>{op, 0, 0, 0, imm0, imm1, 0, 0, W_COPY, 1, 0, 0, 0, 0, 0, 0};
    };
    for (uint32_t k : {0u, 7u}) CHECK(circuit::check_program(program(W_STMT, k, 0).data(), 2, levels, 2, 2, shape) == RSV_OK);
    for (uint32_t k : {8u, 9u, 0x7FFFFFFFu, 0xFFFFFFFFu}) CHECK(circuit::check_program(program(W_STMT, k, 0).data(), 2, levels, 2, 2, shape) == RSV_E_RANGE);
    CHECK(circuit::check_program(program(W_N_OPS, 0, 0).data(), 2, levels, 2, 2, shape) == RSV_E_RANGE);  // the op behind W_STMT is none
    for (uint32_t k : {0u, 15u, 32u, 34u}) CHECK(circuit::check_program(program(W_FLOW, k, 16).data(), 2, levels, 2, 2, shape, false, 3) == RSV_OK);
    for (uint32_t k : {16u, 31u, 35u, 0xFFFFFFFFu}) CHECK(circuit::check_program(program(W_FLOW, k, 16).data(), 2, levels, 2, 2, shape, false, 3) == RSV_E_RANGE);
    for (uint32_t k : {32u, 34u}) CHECK(circuit::check_program(program(W_FLOW, k, 16).data(), 2, levels, 2, 2, shape) == RSV_E_RANGE);

    // check_copies, hashed: the statement 4 .. 11, two copies with one own input each (12, 13), a variable of the hash
    // (14: a tail load), one hint per copy (15, 16); the copies' flow is 2 x 16 records
    using circuit::Instr;
    using circuit::mk_instr;
    std::vector<Instr> origin;
    for (uint32_t k = 0; k < 4; k++) origin.push_back(mk_instr(W_CONST));
    for (uint32_t k = 0; k < 8; k++) origin.push_back(mk_instr(W_STMT, 0, 0, k));
    origin.push_back(mk_instr(W_INPUT, 0, 0, 0));
    origin.push_back(mk_instr(W_INPUT, 0, 0, 0));
    origin.push_back(mk_instr(W_FLOW, 0, 0, 32, 16));
    origin.push_back(mk_instr(W_FLOW, 0, 0, 3, 16));
    origin.push_back(mk_instr(W_WORD, 0, 0, 2));
    for (uint32_t k = 0; k < origin.size(); k++) origin[k].dst = k;
    std::vector<uint8_t> copy_of(17, 0);
    copy_of[13] = 1; copy_of[16] = 1;
    const std::vector<uint32_t> marks{15, 16, 17};
    CHECK(circuit::check_copies(origin, copy_of, marks, 2, 1, false, 32) == RSV_OK);
    CHECK(circuit::check_copies(origin, copy_of, marks, 2, 1) == RSV_E_RANGE);  // not the layout of a program that is not hashed
    {
        std::vector<Instr> o2(origin);
        o2[5].imm[0] = 2;  // word 2 in word 1's place
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1, false, 32) == RSV_E_RANGE);
        o2 = origin;
        o2[11] = mk_instr(W_INPUT, 0, 0, 0);  // an input inside the statement
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1, false, 32) == RSV_E_RANGE);
        o2 = origin;
        o2[12] = mk_instr(W_STMT, 0, 0, 0);  // a statement word among the inputs
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1, false, 32) == RSV_E_RANGE);
        o2 = origin;
        o2[14].imm[0] = 31;  // the hash loads a copy's record
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1, false, 32) == RSV_E_RANGE);
        o2 = origin;
        o2[14] = mk_instr(W_WORD, 0, 0, 2);  // the hash reads the proof
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1, false, 32) == RSV_E_RANGE);
        o2 = origin;
        o2[15].imm[0] = 32;  // a copy loads a record of the tail
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1, false, 32) == RSV_E_RANGE);
        o2 = origin;
        o2[16] = mk_instr(W_STMT, 0, 0, 0);  // a statement word inside a copy
        CHECK(circuit::check_copies(o2, copy_of, marks, 2, 1, false, 32) == RSV_E_RANGE);
    }
    {
        std::vector<uint8_t> c2(copy_of);
        c2[13] = 0;  // copy 1's record given to copy 0
        CHECK(circuit::check_copies(origin, c2, marks, 2, 1, false, 32) == RSV_E_RANGE);
        c2 = copy_of;
        c2[14] = 1;  // the hash belongs to no copy but the first's number
        CHECK(circuit::check_copies(origin, c2, marks, 2, 1, false, 32) == RSV_E_RANGE);
        c2 = copy_of;
        c2[15] = 1;  // copy 1's hint in copy 0's range
        CHECK(circuit::check_copies(origin, c2, marks, 2, 1, false, 32) == RSV_E_RANGE);
        CHECK(circuit::check_copies(origin, copy_of, {13, 16, 17}, 2, 1, false, 32) == RSV_E_RANGE);  // the copies start inside the inputs
        CHECK(circuit::check_copies(origin, copy_of, marks, 2, 0, false, 32) == RSV_E_RANGE);         // a hashed program has own inputs
        CHECK(circuit::check_copies(origin, copy_of, marks, 2, 4096, false, 32) == RSV_E_RANGE);
    }
    printf("refusals: ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && std::string(argv[1]) == "program") return run_program(argv[2], (size_t)atol(argv[3]), argv[4], argv[5]);
    if (argc == 2 && std::string(argv[1]) == "refusals") return run_refusals();
    fprintf(stderr, "usage: statement_host program <hints> <n_fixed> <statement flow> <out> | refusals\n");
    return 2;
}
