// circuit_eval_host.hpp — HOST code, plain C++ (no HIP): a caller's circuit compiled into an EVALUATION program
// (rsv_circuit_program_create_eval, include/rsv.h): from the gate list, the hints and the links between invocations, one
// definition per variable, and the levels in which rsv_circuit_eval_dev (k_circuit_eval.hpp) runs the instructions and
// the Poseidon invocations.  The flow table is user_circuit_host.hpp's: compile() adds the define bits and the links to the
// Tables check() resolved, and the program keeps them.  Included by k_circuit_eval.hpp; compiles on its own with g++ beside user_circuit_host.hpp, so
// a sanitizer build can drive it without a device.
//
// The definition rule (rsv.h has it in full) follows how the reference's constraint system allocates variables
// (constraint_system/src/plonk_with_poseidon.rs:140-283): 0..3 are constants; a hinted variable is its hint; the a / b
// wires of the row that carries an invocation's r3 / r4 wire are the permutation's output; every other variable is the c
// of the first row that does not also read it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "layout.hpp"
#include "user_circuit_host.hpp"

namespace rsv::ceval {

// Instruction: 8 u32 = op, dst, a, b, imm0..3 (k_witness.hpp's layout).  The ops are layout.hpp's W_CONST .. W_BIT, which
// every circuit kernel runs through one function (k_circuit_ops.hpp), and the two below, this program's own.
//   E_INPUT  dst = inputs[imm0]
//   E_GATE   dst = op (a + b) + (1 - op) a b; op = imm0, or with imm2 = 1 (a witness-op row): imm0 where variables[imm1].x != 0, else 0
constexpr uint32_t E_INPUT = 32, E_GATE = 33;
static_assert(E_INPUT >= W_N_OPS, "E_INPUT and E_GATE lie above layout.hpp's ops");
constexpr uint32_t INSTR_WORDS = 8;

struct Program {
    uint32_t n_inputs = 0;
    std::vector<uint32_t> instr;               // [n_instr][8], level after level, by dst within a level
    std::vector<uint32_t> level_offsets;       // [n_levels + 1] into instr
    std::vector<uint32_t> flow_order;          // [n_flow]: the invocations, level after level
    std::vector<uint32_t> flow_level_offsets;  // [n_levels + 1] into flow_order
    ucircuit::Tables tables;                   // check()'s, the flow table with the define bits and the links filled in
    size_t n_levels() const { return level_offsets.empty() ? 0 : level_offsets.size() - 1; }
};

// ucircuit::check()'s refusals first, with its statuses; then RSV_E_NULL for NULL hints with a non-zero count, RSV_E_SIZE
// for n_inputs beyond trace::MAX_WIRE, and RSV_E_RANGE for everything the rule refuses: a hint whose dst, kind, src, imm or
// slot is out of range, a variable with two definitions or none, a link on a half with a wire, to itself or past the
// flow, a dependency cycle.  On an error status `out` is untouched.
inline int compile(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, const uint32_t* witness_ops,
                   size_t n_witness_ops, uint32_t n_vars, uint32_t num_input, const uint32_t* hints, size_t n_hints,
                   const uint32_t* flow_links, uint32_t n_inputs, Program* out) {
    ucircuit::Tables t;
    const int rc = ucircuit::check(gates, n_rows, flow_wires, n_flow, witness_ops, n_witness_ops, n_vars, num_input, &t);
    if (rc != RSV_OK) return rc;
    if (n_hints && !hints) return RSV_E_NULL;
    if (n_inputs > trace::MAX_WIRE) return RSV_E_SIZE;

    enum : uint8_t { D_NONE, D_CONST, D_HINT, D_FLOW, D_ROW };
    std::vector<uint8_t> def(n_vars, D_NONE);
    std::vector<uint32_t> def_at(n_vars, 0);  // the hint, 4 k + the output quarter, or the row
    for (uint32_t v = 0; v < 4 && v < n_vars; v++) def[v] = D_CONST;
    for (size_t i = 0; i < n_hints; i++) {
        const uint32_t dst = hints[i * 4], kind = hints[i * 4 + 1], src = hints[i * 4 + 2], imm = hints[i * 4 + 3];
        if (dst >= n_vars || def[dst] != D_NONE) return RSV_E_RANGE;
        switch (kind) {
        case RSV_HINT_INPUT: if (imm >= n_inputs) return RSV_E_RANGE; break;
        case RSV_HINT_COPY: case RSV_HINT_INV: case RSV_HINT_INV0: case RSV_HINT_QINV: if (src >= n_vars) return RSV_E_RANGE; break;
        case RSV_HINT_CINV: if (src >= n_vars || imm > 1) return RSV_E_RANGE; break;
        case RSV_HINT_COORD: if (src >= n_vars || imm > 3) return RSV_E_RANGE; break;
        case RSV_HINT_BIT: if (src >= n_vars || imm > 31) return RSV_E_RANGE; break;
        default: return RSV_E_RANGE;
        }
        def[dst] = D_HINT;
        def_at[dst] = (uint32_t)i;
    }
    using ucircuit::FLOW_WORDS, ucircuit::FLOW_MASK, ucircuit::FLOW_SWAP_ADDR, ucircuit::FLOW_LINK, ucircuit::FLOW_DEFINES;
    Program p;
    p.n_inputs = n_inputs;
    for (size_t k = 0; k < n_flow; k++) {
        uint32_t* r = t.flow.data() + k * FLOW_WORDS;
        for (uint32_t q = 0; q < 4; q++) {  // output quarter q: half 2 + q / 2, its row's a (q even) or b wire
            if (!((r[FLOW_MASK] >> (2 + q / 2)) & 1u)) continue;
            const uint32_t v = r[4 + q];
            if (def[v] == D_FLOW) return RSV_E_RANGE;  // the output of two rows, or both wires of one
            if (def[v] != D_NONE) continue;            // a constant or a hinted variable stays what it is
            def[v] = D_FLOW;
            def_at[v] = (uint32_t)k * 4 + q;
            r[FLOW_MASK] |= 1u << (FLOW_DEFINES + q);
        }
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t link = flow_links ? flow_links[k * 2 + h] : 0;
            if (!link) continue;
            if (((r[FLOW_MASK] >> h) & 1u) || (link - 1) / 2 >= n_flow || (link - 1) / 2 == k) return RSV_E_RANGE;
            r[FLOW_LINK + h] = link;
        }
    }
    for (size_t i = 0; i < n_rows; i++) {
        const uint32_t a = gates[i * 6], b = gates[i * 6 + 1], v = gates[i * 6 + 2];
        if (def[v] == D_NONE && a != v && b != v) {
            def[v] = D_ROW;
            def_at[v] = (uint32_t)i;
        }
    }
    for (uint32_t v = 0; v < n_vars; v++)
        if (def[v] == D_NONE) return RSV_E_RANGE;

    // One dependency graph: node v < n_vars is a variable, node n_vars + k an invocation.  deps() lists what a node reads.
    const size_t n_nodes = (size_t)n_vars + n_flow;
    auto deps = [&](size_t node, size_t* d) -> int {
        int n = 0;
        if (node >= n_vars) {
            const uint32_t* r = t.flow.data() + (node - n_vars) * FLOW_WORDS;
            for (uint32_t h = 0; h < 2; h++) {
                if ((r[FLOW_MASK] >> h) & 1u) { d[n++] = r[2 * h]; d[n++] = r[2 * h + 1]; }
                else if (r[FLOW_LINK + h]) d[n++] = (size_t)n_vars + (r[FLOW_LINK + h] - 1) / 2;
            }
            if (r[FLOW_SWAP_ADDR]) d[n++] = r[FLOW_SWAP_ADDR];
            return n;
        }
        switch (def[node]) {
        case D_HINT: if (hints[(size_t)def_at[node] * 4 + 1] != RSV_HINT_INPUT) d[n++] = hints[(size_t)def_at[node] * 4 + 2]; break;
        case D_FLOW: d[n++] = (size_t)n_vars + def_at[node] / 4; break;
        case D_ROW: {
            const size_t row = def_at[node];
            d[n++] = gates[row * 6];
            d[n++] = gates[row * 6 + 1];
            if (t.rows[row * ucircuit::ROW_WORDS + 2] & ucircuit::ROW_WITNESS_OP) d[n++] = t.rows[row * ucircuit::ROW_WORDS + 1];
            break;
        }
        default: break;
        }
        return n;
    };
    // Depth = the longest path, by a depth-first walk with a stack of its own.  An output variable is written by its
    // invocation's lane, so it sits at the invocation's level; every other edge costs one level.
    constexpr uint32_t UNSEEN = 0xffffffffu, OPEN = 0xfffffffeu;
    std::vector<uint32_t> level(n_nodes, UNSEEN);
    std::vector<std::pair<size_t, int>> stack;
    uint32_t top = 0;
    for (size_t root = 0; root < n_nodes; root++) {
        if (level[root] != UNSEEN) continue;
        stack.emplace_back(root, 0);
        level[root] = OPEN;
        while (!stack.empty()) {
            const size_t node = stack.back().first;
            size_t d[8];
            const int nd = deps(node, d);
            if (stack.back().second < nd) {
                const size_t next = d[stack.back().second++];
                if (level[next] == OPEN) return RSV_E_RANGE;  // a cycle
                if (level[next] == UNSEEN) {
                    level[next] = OPEN;
                    stack.emplace_back(next, 0);
                }
                continue;
            }
            const uint32_t step = node < n_vars && def[node] == D_FLOW ? 0u : 1u;
            uint32_t l = 0;
            for (int k = 0; k < nd; k++) l = level[d[k]] + step > l ? level[d[k]] + step : l;
            level[node] = l;
            top = l > top ? l : top;
            stack.pop_back();
        }
    }
    const size_t n_levels = (size_t)top + 1;
    p.level_offsets.assign(n_levels + 1, 0);
    p.flow_level_offsets.assign(n_levels + 1, 0);
    for (uint32_t v = 0; v < n_vars; v++)
        if (def[v] != D_FLOW) p.level_offsets[level[v] + 1]++;
    for (size_t k = 0; k < n_flow; k++) p.flow_level_offsets[level[n_vars + k] + 1]++;
    for (size_t l = 0; l < n_levels; l++) {
        p.level_offsets[l + 1] += p.level_offsets[l];
        p.flow_level_offsets[l + 1] += p.flow_level_offsets[l];
    }
    std::vector<uint32_t> at(p.level_offsets.begin(), p.level_offsets.end() - 1), fat(p.flow_level_offsets.begin(), p.flow_level_offsets.end() - 1);
    p.instr.assign((size_t)p.level_offsets[n_levels] * INSTR_WORDS, 0);
    p.flow_order.assign(n_flow, 0);
    for (size_t k = 0; k < n_flow; k++) p.flow_order[fat[level[n_vars + k]]++] = (uint32_t)k;
    for (uint32_t v = 0; v < n_vars; v++) {
        if (def[v] == D_FLOW) continue;
        uint32_t* w = p.instr.data() + (size_t)at[level[v]]++ * INSTR_WORDS;
        w[1] = v;
        if (def[v] == D_CONST) {
            w[0] = W_CONST;
            if (v) w[3 + v] = 1;  // 1, i, j
        } else if (def[v] == D_HINT) {
            const uint32_t* h = hints + (size_t)def_at[v] * 4;
            constexpr uint32_t op_of[8] = {E_INPUT, W_COPY, W_INV, W_INV0, W_QINV, W_CINV, W_COORD, W_BIT};
            w[0] = op_of[h[1]];
            if (h[1] != RSV_HINT_INPUT) w[2] = h[2];
            if (h[1] == RSV_HINT_INPUT || h[1] >= RSV_HINT_CINV) w[4] = h[3];
        } else {
            const size_t row = def_at[v];
            const uint32_t a = gates[row * 6], b = gates[row * 6 + 1], op = t.rows[row * ucircuit::ROW_WORDS];
            w[2] = a;
            w[3] = b;
            if (t.rows[row * ucircuit::ROW_WORDS + 2] & ucircuit::ROW_WITNESS_OP) {
                w[0] = E_GATE; w[4] = op; w[5] = t.rows[row * ucircuit::ROW_WORDS + 1]; w[6] = 1;
            } else if (op == 1) w[0] = W_ADD;
            else if (op == 0) w[0] = W_MUL;
            else if (b == 0) { w[0] = W_MULC; w[3] = 0; w[4] = op; }
            else { w[0] = E_GATE; w[4] = op; }
        }
    }
    p.tables = std::move(t);
    if (out) *out = std::move(p);
    return RSV_OK;
}

}  // namespace rsv::ceval
