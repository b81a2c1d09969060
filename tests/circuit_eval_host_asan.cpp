// circuit_eval_host_asan.cpp — stand-alone driver of recursive-stwo_amd/csrc/circuit_eval_host.hpp (and user_circuit_host.hpp,
// trace_host.hpp under it) for a g++ -fsanitize=address,undefined build: tests/test_circuit_eval_host.py compiles and runs
// it.  No HIP, no device.
//
//   circuit_eval_host_asan file <circuit.bin> <seed> <rounds>
//        a recorded circuit: header {magic, n_rows, n_flow, n_ops, n_vars, num_input, n_hints, n_inputs}, gates, flow wires,
//        witness ops, hints, links.  compile() must accept it, the program must point inside the arrays and respect its own
//        levels, and every single-word corruption drawn from the seed must be refused or leave such a program.
//   circuit_eval_host_asan adversarial
//        hand-made arrays for every refusal: out-of-range indices, a cycle, a doubly defined variable, a self-link, empty hints.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../recursive-stwo_amd/csrc/circuit_eval_host.hpp"

using namespace rsv::ceval;
using namespace rsv::ucircuit;  // the flow table is user_circuit_host.hpp's; the ops below E_INPUT are layout.hpp's
using rsv::W_ADD, rsv::W_MUL, rsv::W_MULC, rsv::W_CINV, rsv::W_COORD, rsv::W_BIT;

#define REQUIRE(x)                                                          \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

struct Circuit {
    std::vector<uint32_t> gates, flow, ops, hints, links;
    uint32_t n_vars = 0, num_input = 3, n_inputs = 0;
    int run(Program* p) const {
        return compile(gates.data(), gates.size() / 6, flow.data(), flow.size() / 5, ops.data(), ops.size() / 3, n_vars, num_input, hints.data(),
                       hints.size() / 4, links.empty() ? nullptr : links.data(), n_inputs, p);
    }
};

// every index inside its array, every variable defined once, every read at a strictly lower level
static void program_is_sound(const Circuit& c, const Program& p) {
    const size_t n_flow = c.flow.size() / 5, n_levels = p.n_levels(), n_instr = p.instr.size() / INSTR_WORDS;
    REQUIRE(n_levels >= 1 && p.flow_level_offsets.size() == n_levels + 1 && p.flow_order.size() == n_flow);
    const std::vector<uint32_t>& flow = p.tables.flow;
    REQUIRE(flow.size() == n_flow * FLOW_WORDS && p.tables.rows.size() == c.gates.size() / 6 * ROW_WORDS);
    REQUIRE(p.level_offsets[0] == 0 && p.level_offsets[n_levels] == n_instr && p.flow_level_offsets[0] == 0 && p.flow_level_offsets[n_levels] == n_flow);
    std::vector<int64_t> var_level(c.n_vars, -1), flow_level(n_flow, -1);
    for (size_t l = 0; l < n_levels; l++) {
        REQUIRE(p.level_offsets[l] <= p.level_offsets[l + 1] && p.flow_level_offsets[l] <= p.flow_level_offsets[l + 1]);
        for (size_t i = p.level_offsets[l]; i < p.level_offsets[l + 1]; i++) {
            const uint32_t dst = p.instr[i * INSTR_WORDS + 1];
            REQUIRE(dst < c.n_vars && var_level[dst] < 0);
            var_level[dst] = (int64_t)l;
        }
        for (size_t j = p.flow_level_offsets[l]; j < p.flow_level_offsets[l + 1]; j++) {
            const uint32_t k = p.flow_order[j];
            REQUIRE(k < n_flow && flow_level[k] < 0);
            flow_level[k] = (int64_t)l;
            for (int q = 0; q < 4; q++) {  // the variable output quarter q defines: word 4 + q where its define bit is set
                if (!((flow[k * FLOW_WORDS + FLOW_MASK] >> (FLOW_DEFINES + q)) & 1u)) continue;
                const uint32_t v = flow[k * FLOW_WORDS + 4 + q];
                REQUIRE(v >= 4 && v < c.n_vars && var_level[v] < 0);
                var_level[v] = (int64_t)l;
            }
        }
    }
    for (uint32_t v = 0; v < c.n_vars; v++) REQUIRE(var_level[v] >= 0);
    for (size_t l = 0; l < n_levels; l++) {
        for (size_t i = p.level_offsets[l]; i < p.level_offsets[l + 1]; i++) {
            const uint32_t* w = p.instr.data() + i * INSTR_WORDS;
            const uint32_t op = w[0];
            REQUIRE(op <= W_BIT || op == E_INPUT || op == E_GATE);
            const bool two = op == W_ADD || op == W_MUL || op == E_GATE, one = two || (op >= W_MULC && op <= W_BIT);
            if (one) REQUIRE(w[2] < c.n_vars && var_level[w[2]] < (int64_t)l);
            if (two) REQUIRE(w[3] < c.n_vars && var_level[w[3]] < (int64_t)l);
            if (op == E_GATE && w[6]) REQUIRE(w[5] < c.n_vars && var_level[w[5]] < (int64_t)l);
            if (op == E_INPUT) REQUIRE(w[4] < c.n_inputs);
            if (op == W_CINV) REQUIRE(w[4] <= 1);
            if (op == W_COORD) REQUIRE(w[4] <= 3);
            if (op == W_BIT) REQUIRE(w[4] <= 31);
        }
    }
    for (size_t k = 0; k < n_flow; k++) {
        const uint32_t* r = flow.data() + k * FLOW_WORDS;
        REQUIRE(r[FLOW_MASK] < (16u << FLOW_DEFINES) && r[FLOW_SWAP_ADDR] < c.n_vars);
        for (int q = 0; q < 4; q++)  // a define bit only on an output half that has a wire
            if ((r[FLOW_MASK] >> (FLOW_DEFINES + q)) & 1u) REQUIRE((r[FLOW_MASK] >> (2 + q / 2)) & 1u);
        if (r[FLOW_SWAP_ADDR]) REQUIRE(var_level[r[FLOW_SWAP_ADDR]] < flow_level[k]);
        for (int h = 0; h < 2; h++) {
            if ((r[FLOW_MASK] >> h) & 1u) {
                REQUIRE(r[2 * h] < c.n_vars && r[2 * h + 1] < c.n_vars && r[FLOW_LINK + h] == 0);
                REQUIRE(var_level[r[2 * h]] < flow_level[k] && var_level[r[2 * h + 1]] < flow_level[k]);
            } else if (r[FLOW_LINK + h]) {  // a link sits only on a half without a wire
                const uint32_t from = (r[FLOW_LINK + h] - 1) / 2;
                REQUIRE(from < n_flow && flow_level[from] < flow_level[k]);
            }
        }
    }
}

// four constant rows; inputs 4 and 5; 6 = 4 + 5; Poseidon rows for (6, 4) -> wire 7 and for the output (8, 9) -> wire 10; 11 = 8 * 9;
// a second invocation fed by the first one's ignored r4 through a link, bound output (12, 13) -> wire 14, swap address 4
static Circuit tiny() {
    Circuit c;
    for (uint32_t k = 0; k < 4; k++) c.gates.insert(c.gates.end(), {k, 0, k, 1, 0, 0});
    c.gates.insert(c.gates.end(), {4, 0, 4, 1, 0, 1});
    c.gates.insert(c.gates.end(), {4, 5, 6, 1, 0, 0});
    c.gates.insert(c.gates.end(), {6, 4, 7, 0, 7, 0});
    c.gates.insert(c.gates.end(), {8, 9, 10, 0, 10, 0});
    c.gates.insert(c.gates.end(), {8, 9, 11, 0, 0, 0});
    c.gates.insert(c.gates.end(), {12, 13, 14, 0, 14, 0});
    c.flow = {7, 0, 10, 0, 0, /**/ 0, 0, 14, 0, 4};
    c.links = {0, 0, /**/ 2, 0};
    c.hints = {4, RSV_HINT_INPUT, 0, 0, /**/ 5, RSV_HINT_INPUT, 0, 1};
    c.n_vars = 15;
    c.n_inputs = 2;
    return c;
}

static int adversarial() {
    Program p;
    Circuit c = tiny();
    REQUIRE(c.run(&p) == RSV_OK);
    program_is_sound(c, p);
    REQUIRE(p.instr.size() / INSTR_WORDS == 15 - 4 && c.run(nullptr) == RSV_OK);
    const uint32_t* r = p.tables.flow.data();  // invocation 0 defines 8 and 9, invocation 1 defines 12 and 13 and links r1 to 0's r4
    REQUIRE(r[4] == 8 && r[5] == 9 && r[FLOW_MASK] == (5u | 3u << FLOW_DEFINES) && r[FLOW_LINK] == 0 && r[FLOW_LINK + 1] == 0);
    r += FLOW_WORDS;
    REQUIRE(r[4] == 12 && r[5] == 13 && r[FLOW_MASK] == (4u | 3u << FLOW_DEFINES) && r[FLOW_SWAP_ADDR] == 4 && r[FLOW_LINK] == 2 && r[FLOW_LINK + 1] == 0);
    const Program kept = p;
    auto refused = [&](const Circuit& bad, int code) {
        REQUIRE(bad.run(&p) == code);
        REQUIRE(p.instr == kept.instr && p.tables.flow == kept.tables.flow && p.tables.rows == kept.tables.rows &&
                p.flow_order == kept.flow_order);  // nothing is written on a refusal
    };
    Circuit b = c; b.gates.clear(); refused(b, RSV_E_SIZE);                // user_circuit_host.hpp's checks come first
    b = c; b.n_vars = 14; refused(b, RSV_E_RANGE);
    REQUIRE(compile(c.gates.data(), c.gates.size() / 6, c.flow.data(), 2, nullptr, 0, c.n_vars, 3, nullptr, 2, c.links.data(), 2, &p) == RSV_E_NULL);
    b = c; b.n_inputs = rsv::trace::MAX_WIRE + 1; refused(b, RSV_E_SIZE);
    b = c; b.hints[0] = 15; refused(b, RSV_E_RANGE);                       // dst out of range
    b = c; b.hints[1] = 8; refused(b, RSV_E_RANGE);                        // an unknown kind
    b = c; b.hints[3] = 2; refused(b, RSV_E_RANGE);                        // a slot >= n_inputs
    b = c; b.hints[1] = RSV_HINT_COPY; b.hints[2] = 15; refused(b, RSV_E_RANGE);  // src out of range
    b = c; b.hints[1] = RSV_HINT_CINV; b.hints[2] = 5; b.hints[3] = 2; refused(b, RSV_E_RANGE);
    b = c; b.hints[1] = RSV_HINT_COORD; b.hints[2] = 5; b.hints[3] = 4; refused(b, RSV_E_RANGE);
    b = c; b.hints[1] = RSV_HINT_BIT; b.hints[2] = 5; b.hints[3] = 32; refused(b, RSV_E_RANGE);
    b = c; b.hints.insert(b.hints.end(), {5, RSV_HINT_COPY, 4, 0}); refused(b, RSV_E_RANGE);   // a doubly defined variable
    b = c; b.hints.insert(b.hints.end(), {1, RSV_HINT_COPY, 4, 0}); refused(b, RSV_E_RANGE);   // ... a constant
    b = c; b.hints.clear(); refused(b, RSV_E_RANGE);                       // empty hints: 4 and 5 have no definition
    b = c; b.hints[1] = RSV_HINT_COPY; b.hints[2] = 5; b.hints[5] = RSV_HINT_COPY; b.hints[6] = 4; refused(b, RSV_E_RANGE);  // a cycle of hints
    b = c; b.hints[5] = RSV_HINT_QINV; b.hints[6] = 11; refused(b, RSV_E_RANGE);   // a cycle through an invocation: 5 <- 11 <- 8 <- invocation 0 <- 6 <- 5
    b = c; b.links[2] = 3; refused(b, RSV_E_RANGE);                        // a self-link
    b = c; b.links[2] = 5; refused(b, RSV_E_RANGE);                        // k' >= n_flow
    b = c; b.links[0] = 3; refused(b, RSV_E_RANGE);                        // a link on a half that has a wire
    b = c; b.links[1] = 4; b.links[2] = 2; refused(b, RSV_E_RANGE);        // a cycle of links
    b = c; b.flow[7] = 10; refused(b, RSV_E_RANGE);                        // one row the output of two invocations
    b = c; b.gates[9 * 6] = 13; refused(b, RSV_E_RANGE);                   // both wires of an output row are one variable
    b = c; b.links.clear(); REQUIRE(b.run(&p) == RSV_OK); program_is_sound(b, p);   // NULL links: the half is the caller's
    std::puts("adversarial ok");
    return 0;
}

static int recorded(const char* path, uint64_t seed, int rounds) {
    std::FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    uint32_t h[8];
    REQUIRE(std::fread(h, 4, 8, f) == 8 && h[0] == 0x43455631u);
    Circuit c;
    c.gates.resize((size_t)h[1] * 6); c.flow.resize((size_t)h[2] * 5); c.ops.resize((size_t)h[3] * 3);
    c.n_vars = h[4]; c.num_input = h[5];
    c.hints.resize((size_t)h[6] * 4); c.n_inputs = h[7]; c.links.resize((size_t)h[2] * 2);
    for (std::vector<uint32_t>* a : {&c.gates, &c.flow, &c.ops, &c.hints, &c.links}) REQUIRE(std::fread(a->data(), 4, a->size(), f) == a->size());
    std::fclose(f);
    Program p;
    REQUIRE(c.run(&p) == RSV_OK);
    program_is_sound(c, p);
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    int refusals = 0;
    for (int r = 0; r < rounds; r++) {
        Circuit b = c;
        std::vector<uint32_t>* arr[5] = {&b.gates, &b.flow, &b.hints, &b.links, &b.ops};
        std::vector<uint32_t>& a = *arr[next() % (b.ops.empty() ? 4 : 5)];
        const uint32_t kinds[4] = {next() % (c.n_vars + 2), c.n_vars, 0xffffffffu, next()};
        a[next() % a.size()] = kinds[next() % 4];
        Program pb;
        const int rc = b.run(&pb);
        if (rc == RSV_OK) program_is_sound(b, pb);
        else {
            REQUIRE((rc == RSV_E_RANGE || rc == RSV_E_SIZE) && pb.instr.empty() && pb.tables.flow.empty() && pb.tables.rows.empty());
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
