// user_circuit_host_asan.cpp — stand-alone driver of recursive-stwo_amd/csrc/user_circuit_host.hpp (and trace_host.hpp under
// it) for a g++ -fsanitize=address,undefined build: tests/test_user_circuit_host.py compiles and runs it.  No HIP, no device.
//
//   user_circuit_host_asan file <circuit.bin>   a recorded circuit: header {magic, n_rows, n_flow, n_ops, n_vars, num_input},
//                                               gates, flow wires, witness ops.  check() must accept it, its tables must
//                                               point inside the arrays, and every single-word corruption drawn from the
//                                               seed must be refused or leave tables that still point inside.
//   user_circuit_host_asan adversarial          hand-made arrays for every refusal.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../recursive-stwo_amd/csrc/user_circuit_host.hpp"

using namespace rsv::ucircuit;

#define REQUIRE(x)                                                          \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

struct Circuit {
    std::vector<uint32_t> gates, flow, ops;
    uint32_t n_vars = 0, num_input = 3;
    int run(Tables* t) const {
        return check(gates.data(), gates.size() / 6, flow.data(), flow.size() / 5, ops.data(), ops.size() / 3, n_vars, num_input, t);
    }
};

static void tables_point_inside(const Circuit& c, const Tables& t) {
    REQUIRE(t.rows.size() == c.gates.size() / 6 * ROW_WORDS && t.flow.size() == c.flow.size() / 5 * FLOW_WORDS);
    for (size_t i = 0; i < t.rows.size() / ROW_WORDS; i++) {
        REQUIRE(t.rows[i * ROW_WORDS] < rsv::trace::MP && t.rows[i * ROW_WORDS + 1] < c.n_vars);
        REQUIRE((t.rows[i * ROW_WORDS + 2] & ~(ROW_M31 | ROW_WITNESS_OP)) == 0);
    }
    for (size_t f = 0; f < t.flow.size() / FLOW_WORDS; f++) {
        for (int k = 0; k < 8; k++) REQUIRE(t.flow[f * FLOW_WORDS + k] < c.n_vars);
        REQUIRE(t.flow[f * FLOW_WORDS + FLOW_MASK] < 16 && t.flow[f * FLOW_WORDS + FLOW_SWAP_ADDR] < c.n_vars);
        REQUIRE(t.flow[f * FLOW_WORDS + FLOW_LINK] == 0 && t.flow[f * FLOW_WORDS + FLOW_LINK + 1] == 0);  // an evaluation program's
    }
}

// four constant rows, an add, two Poseidon gates, one invocation (5 -> 6, swap address 4): 7 variables
static Circuit tiny() {
    Circuit c;
    for (uint32_t k = 0; k < 4; k++) c.gates.insert(c.gates.end(), {k, 0, k, 1, 0, 0});
    c.gates.insert(c.gates.end(), {1, 2, 4, 1, 0, 0});
    c.gates.insert(c.gates.end(), {4, 4, 5, 0, 5, 0});
    c.gates.insert(c.gates.end(), {4, 1, 6, 0, 6, 0});
    c.flow = {5, 0, 6, 0, 4};
    c.ops = {4, 4, 77};
    c.n_vars = 7;
    return c;
}

static int adversarial() {
    Tables t;
    Circuit c = tiny();
    REQUIRE(c.run(&t) == RSV_OK);
    tables_point_inside(c, t);
    REQUIRE(t.rows[4 * ROW_WORDS] == 77 && t.rows[4 * ROW_WORDS + 1] == 4 && t.rows[4 * ROW_WORDS + 2] == ROW_WITNESS_OP);
    REQUIRE(t.flow[0] == 4 && t.flow[1] == 4 && t.flow[4] == 4 && t.flow[5] == 1 && t.flow[FLOW_MASK] == 5 && t.flow[FLOW_SWAP_ADDR] == 4);
    REQUIRE(c.run(nullptr) == RSV_OK);
    const Tables kept = t;
    auto refused = [&](const Circuit& bad, int code) {
        REQUIRE(bad.run(&t) == code);
        REQUIRE(t.rows == kept.rows && t.flow == kept.flow);  // nothing is written on a refusal
    };
    REQUIRE(check(nullptr, 7, c.flow.data(), 1, nullptr, 0, 7, 3, &t) == RSV_E_NULL);
    REQUIRE(check(c.gates.data(), 7, nullptr, 1, nullptr, 0, 7, 3, &t) == RSV_E_NULL);
    REQUIRE(check(c.gates.data(), 7, c.flow.data(), 1, nullptr, 1, 7, 3, &t) == RSV_E_NULL);
    REQUIRE(check(c.gates.data(), 7, c.flow.data(), 1, nullptr, 0, 7, 3, &t) == RSV_OK);
    t = kept;
    REQUIRE(check(c.gates.data(), 0, c.flow.data(), 1, nullptr, 0, 7, 3, &t) == RSV_E_SIZE);
    REQUIRE(check(c.gates.data(), 7, c.flow.data(), 0, nullptr, 0, 7, 3, &t) == RSV_E_SIZE);
    REQUIRE(check(c.gates.data(), ((size_t)1 << RSV_MAX_WITNESS_LOG) + 1, c.flow.data(), 1, nullptr, 0, 7, 3, &t) == RSV_E_SIZE);
    REQUIRE(check(c.gates.data(), 7, c.flow.data(), (size_t)1 << 22, nullptr, 0, 7, 3, &t) == RSV_E_SIZE);
    Circuit b = c; b.n_vars = rsv::trace::MAX_WIRE + 1; refused(b, RSV_E_SIZE);
    b = c; b.n_vars = 6; refused(b, RSV_E_RANGE);                      // a wire >= n_vars
    b = c; b.gates[4 * 6 + 1] = 7; refused(b, RSV_E_RANGE);
    b = c; b.ops[1] = 7; refused(b, RSV_E_RANGE);                      // a bit variable >= n_vars
    b = c; b.ops[0] = 7; refused(b, RSV_E_RANGE);                      // a witness-op row >= n_rows
    b = c; b.flow[4] = 9; refused(b, RSV_E_RANGE);                     // a swap address >= n_vars
    b = c; b.gates[2 * 6 + 5] = 1; refused(b, RSV_E_RANGE);            // a constant row is not (k, 0, k, 1, 0, 0)
    b = c; b.gates.resize(3 * 6); refused(b, RSV_E_RANGE);            // fewer than four rows
    b = c; b.num_input = 2; refused(b, RSV_E_RANGE);
    b = c; b.num_input = 7; refused(b, RSV_E_RANGE);
    b = c; b.flow[1] = 4; refused(b, RSV_E_RANGE);                     // a flow wire no row carries
    b = c; b.gates[6 * 6 + 4] = 5; b.flow[2] = 0; refused(b, RSV_E_RANGE);  // a Poseidon wire two rows carry
    b = c; b.gates.insert(b.gates.end(), {5, 0, 5, 1, 0, 0}); refused(b, RSV_E_RANGE);  // a Poseidon wire used more than once
    b = c; b.num_input = 5; refused(b, RSV_E_RANGE);                   // ... by being a public input
    b = c; b.flow[4] = 5; refused(b, RSV_E_RANGE);                     // ... or a swap address
    std::puts("adversarial ok");
    return 0;
}

static int recorded(const char* path, uint64_t seed, int rounds) {
    std::FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    uint32_t h[6];
    REQUIRE(std::fread(h, 4, 6, f) == 6 && h[0] == 0x55435631u);
    Circuit c;
    c.gates.resize((size_t)h[1] * 6); c.flow.resize((size_t)h[2] * 5); c.ops.resize((size_t)h[3] * 3);
    c.n_vars = h[4]; c.num_input = h[5];
    REQUIRE(std::fread(c.gates.data(), 4, c.gates.size(), f) == c.gates.size());
    REQUIRE(std::fread(c.flow.data(), 4, c.flow.size(), f) == c.flow.size());
    REQUIRE(std::fread(c.ops.data(), 4, c.ops.size(), f) == c.ops.size());
    std::fclose(f);
    Tables t;
    REQUIRE(c.run(&t) == RSV_OK);
    tables_point_inside(c, t);
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    int refusals = 0;
    for (int r = 0; r < rounds; r++) {
        Circuit b = c;
        std::vector<uint32_t>* arr[3] = {&b.gates, &b.flow, &b.ops};
        std::vector<uint32_t>& a = *arr[next() % (b.ops.empty() ? 2 : 3)];
        const uint32_t kinds[4] = {next() % (c.n_vars + 2), c.n_vars, 0xffffffffu, next()};
        a[next() % a.size()] = kinds[next() % 4];
        Tables tb;
        const int rc = b.run(&tb);
        if (rc == RSV_OK) tables_point_inside(b, tb);
        else {
            REQUIRE((rc == RSV_E_RANGE || rc == RSV_E_SIZE) && tb.rows.empty() && tb.flow.empty());
            refusals++;
        }
    }
    std::printf("recorded ok: %d of %d corruptions refused\n", refusals, rounds);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "adversarial") return adversarial();
    if (argc == 5 && std::string(argv[1]) == "file") return recorded(argv[2], std::strtoull(argv[3], nullptr, 10), std::atoi(argv[4]));
    std::fprintf(stderr, "usage: %s adversarial | file <circuit.bin> <seed> <rounds>\n", argv[0]);
    return 2;
}
