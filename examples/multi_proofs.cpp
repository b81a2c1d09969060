// examples/multi_proofs.cpp — batch counterpart of the reference's examples/multi-proofs/src/main.rs:40-139: every
// file named on the command line is one serialized proof of the recursion chain (public inputs (1,1), (2,i), (3,u),
// :49-57), verified under the configuration the reference's main() names for that level (:173-295; the file name
// `levelK-*.bin` selects it, anything else is verified under standard_config); all of them go through one pipelined
// call that takes the host buffers as they are.
//
//   g++ -std=c++17 -O1 -o multi_proofs examples/multi_proofs.cpp -Lrecursive-stwo_amd/csrc -lrsv_hip \
//       -Wl,-rpath,$PWD/recursive-stwo_amd/csrc -Wl,-rpath,/opt/rocm/lib
//   ./multi_proofs tests/golden/proofs/level*.bin
//
// --own-inputs: the RECURSING step over a batch in which every proof has its own statement.  The files are proofs of ONE
// shape and configuration; each may be followed by `:v`, the M31 value of its own public input (1 .. 2^31 - 2; default 1).
// The records are (2, i), (3, u) — shared, constants of the circuit — and (1, v): the proof's own, a PublicInput variable
// of the circuit that verifies it.  One program, built from the first file, serves every proof; variable 4 of proof k's
// witness is its v, and the next proof would carry it as its fourth public input.
//   ./multi_proofs --own-inputs tests/golden/proofs/level10-1.bin tests/golden/proofs/level11-1.bin:2
// accepts the first (its statement is (1, 1)) and rejects the second (stage 3: the logup balance does not close under (1, 2)).
// --hash-inputs: the same step with a program whose statement is the DIGEST of the proof's own records: eight words
// (variables 4 .. 11 of the witness) whatever the number of records, so that a tree of such steps keeps its statement's
// size; the record itself is variable 12.
//   ./multi_proofs --hash-inputs tests/golden/proofs/level10-1.bin tests/golden/proofs/level11-1.bin
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

#include "../recursive-stwo_amd/host/recursive_stwo.hpp"

using namespace recursive_stwo;

// examples/multi-proofs/src/main.rs:173-196
static const PcsConfig standard_config{20, FriConfig::make(8, 5, 16)}, fast_prover_config{20, FriConfig::make(8, 1, 80)},
    fast_prover2_config{20, FriConfig::make(8, 3, 27)}, fast_verifier_config{23, FriConfig::make(8, 7, 11)},
    fast_verifier2_config{20, FriConfig::make(8, 8, 10)}, fast_verifier3_config{28, FriConfig::make(7, 9, 8)};
// the configuration levelK was PROVEN under = the one the next demo_recurse call verifies it with (:198-295)
static PcsConfig config_of_level(int k) {
    switch (k) {
        case 1: case 4: return fast_prover_config;
        case 2: case 5: return fast_prover2_config;
        case 8: case 9: return fast_verifier_config;
        case 10: case 11: return fast_verifier2_config;
        case 12: case 13: case 14: return fast_verifier3_config;
        default: return standard_config;  // recursive_proof_16_15, level3, level6, level7
    }
}

static int own_inputs(int argc, char** argv, bool hashed) {
    std::vector<std::vector<uint8_t>> proofs;
    std::vector<Inputs> own;
    PcsConfig config = standard_config;
    for (int i = 2; i < argc; i++) {
        std::string name = argv[i];
        uint32_t v = 1;
        const size_t colon = name.rfind(':');
        if (colon != std::string::npos) { v = (uint32_t)strtoul(name.c_str() + colon + 1, nullptr, 10); name.resize(colon); }
        const size_t at = name.rfind("level");
        if (i == 2) config = config_of_level(at == std::string::npos ? 0 : atoi(name.c_str() + at + 5));
        std::ifstream f(name, std::ios::binary);
        if (!f) { fprintf(stderr, "cannot read %s\n", name.c_str()); return 2; }
        proofs.emplace_back((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        own.push_back({{1, QM31{v, 0, 0, 0}}});
    }
    if (proofs.empty()) return 0;
    const Inputs fixed = {{2, QM31{0, 1, 0, 0}}, {3, QM31{0, 0, 1, 0}}};
    Inputs of_template = fixed;
    of_template.push_back(own[0][0]);
    const WitnessProgram program = WitnessProgram::build_inputs(proofs[0], config, of_template, fixed.size(), 1, {}, hashed);
    std::vector<uint8_t> accept, reason;
    const auto variables = program.variables(proofs, fixed, own, accept, reason);
    int bad = 0;
    for (size_t i = 0; i < proofs.size(); i++) {
        if (accept[i] && hashed) {
            printf("%-40s accepted: %u variables, variable 12 = %u, statement =", argv[i + 2], program.n_vars, (unsigned)variables[i][12][0]);
            for (int k = 0; k < 8; k++) printf(" %u", (unsigned)variables[i][4 + k][0]);
            printf("\n");
        } else if (accept[i]) printf("%-40s accepted: %u variables, variable 4 = %u\n", argv[i + 2], program.n_vars, (unsigned)variables[i][4][0]);
        else printf("%-40s REJECTED (stage %u)\n", argv[i + 2], (unsigned)reason[i]);
        bad += !accept[i];
    }
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--own-inputs") return own_inputs(argc, argv, false);
    if (argc > 1 && std::string(argv[1]) == "--hash-inputs") return own_inputs(argc, argv, true);
    std::vector<std::vector<uint8_t>> proofs;
    std::vector<PcsConfig> configs;
    for (int i = 1; i < argc; i++) {
        const std::string name = argv[i];
        const size_t at = name.rfind("level");
        configs.push_back(config_of_level(at == std::string::npos ? 0 : atoi(name.c_str() + at + 5)));
        std::ifstream f(argv[i], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        proofs.emplace_back((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    }
    const Inputs inputs = {{1, QM31{1, 0, 0, 0}}, {2, QM31{0, 1, 0, 0}}, {3, QM31{0, 0, 1, 0}}};
    std::vector<uint8_t> accept, reason;
    if (proofs.empty()) return 0;
    Verifier::verify_batch(proofs, configs, inputs, accept, reason);
    int bad = 0;
    for (size_t i = 0; i < proofs.size(); i++) {
        printf("%-40s %s (stage %u)\n", argv[i + 1], accept[i] ? "accepted" : "REJECTED", (unsigned)reason[i]);
        bad += !accept[i];
    }
    return bad ? 1 : 0;
}
