// user_circuit_host.hpp — HOST code, plain C++ (no HIP): a caller's own Plonk-with-Poseidon circuit as the chain's program
// (rsv_circuit_program_create, include/rsv.h).  check() is everything the library asks of the arrays before it keeps
// them, and, given `out`, resolves them into the two device tables rsv_circuit_check_dev / rsv_circuit_flow_dev read
// (k_user_circuit.hpp) and, with what circuit_eval_host.hpp adds to the flow table, rsv_circuit_eval_dev (k_circuit_eval.hpp).  Included by user_circuit_api.inc; compiles on its own with g++ beside trace_host.hpp, so a
// sanitizer build can drive it without a device.  The circuit_*.hpp files are something else: the library's mirror of the
// reference's verifier gadgets.
//
//   check_arithmetics            constraint_system/src/plonk_with_poseidon.rs:337-381
//   check_poseidon_invocations   :468-519
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "trace_host.hpp"

namespace rsv::ucircuit {

// Row table, [n_rows][4] (one 16-byte load per lane): the row's op mod P — at a witness-op row the constant the op takes
// when the bit is set —, the bit's variable, ROW_* flags, 0.
constexpr uint32_t ROW_WORDS = 4, ROW_M31 = 1u, ROW_WITNESS_OP = 2u;
// Flow table, [n_flow][12] (three 16-byte loads per lane), the one table of k_uc_flow and of the evaluation kernels:
// (a_wire, b_wire) of the row that carries the poseidon_wire of r1, r2, r3, r4 (zeros for wire 0), a mask with bit h set
// where half h has a wire, the swap address, then what only an evaluation program has (check() leaves zeros,
// ceval::compile fills them in, k_uc_flow reads neither): mask bit FLOW_DEFINES + q set where the invocation defines the
// variable in word 4 + q, and the links of the input halves r1, r2 (0: none, else 1 + 2 k' + h').
constexpr uint32_t FLOW_WORDS = 12, FLOW_MASK = 8, FLOW_SWAP_ADDR = 9, FLOW_LINK = 10, FLOW_DEFINES = 4;

struct Tables {
    std::vector<uint32_t> rows, flow;
};

// Everything is checked before anything is written: on an error status `out` (may be NULL: the checks only) is untouched.
// RSV_E_NULL: a NULL array with a non-zero count.  RSV_E_SIZE: zero rows or flow, log sizes beyond RSV_MAX_WITNESS_LOG,
// n_vars beyond trace::MAX_WIRE.  RSV_E_RANGE: a wire, bit variable or swap address >= n_vars (a witness-op row >= n_rows),
// the four constant rows absent, num_input < 3 or >= n_vars, a non-zero flow wire that is not the poseidon_wire of
// exactly one row, a Poseidon wire used more than once (the assert of populate_logup_arguments, as trace::preprocessed).
inline int check(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, const uint32_t* witness_ops,
                 size_t n_witness_ops, uint32_t n_vars, uint32_t num_input, Tables* out) {
    if ((n_rows && !gates) || (n_flow && !flow_wires) || (n_witness_ops && !witness_ops)) return RSV_E_NULL;
    uint32_t lp = 0, lq = 0;
    const int rc = trace::log_sizes(n_rows, n_flow, lp, lq);
    if (rc != RSV_OK) return rc;
    if (n_vars > trace::MAX_WIRE) return RSV_E_SIZE;
    if (n_rows < 4 || num_input < 3 || num_input >= n_vars) return RSV_E_RANGE;
    for (uint32_t k = 0; k < 4; k++) {  // (k, 0, k, op 1): variables 0..3 are 0, 1, i, j
        const uint32_t* g = gates + (size_t)k * 6;
        if (g[0] != k || g[1] != 0 || g[2] != k || g[3] != 1 || g[4] != 0 || g[5] != 0) return RSV_E_RANGE;
    }
    for (size_t i = 0; i < n_rows; i++)
        for (int k : {0, 1, 2, 4})
            if (gates[i * 6 + k] >= n_vars) return RSV_E_RANGE;
    for (size_t i = 0; i < n_flow * 5; i++)
        if (flow_wires[i] >= n_vars) return RSV_E_RANGE;
    for (size_t i = 0; i < n_witness_ops; i++)
        if (witness_ops[i * 3] >= n_rows || witness_ops[i * 3 + 1] >= n_vars) return RSV_E_RANGE;

    // uses of every variable as populate_logup_arguments counts them, and the row of every Poseidon wire (+ 1; 0: none)
    std::vector<uint32_t> uses(n_vars, 0), row_of(n_vars, 0);
    for (size_t i = 0; i < n_rows; i++) {
        for (int k = 0; k < 3; k++) uses[gates[i * 6 + k]]++;
        const uint32_t w = gates[i * 6 + 4];
        if (w) {
            if (row_of[w]) row_of[w] = UINT32_MAX;  // carried by more than one row
            else row_of[w] = (uint32_t)i + 1;
        }
    }
    for (uint32_t k = 1; k <= num_input; k++) uses[k]++;
    for (size_t f = 0; f < n_flow; f++) uses[flow_wires[f * 5 + 4]]++;
    for (size_t f = 0; f < n_flow; f++)
        for (int h = 0; h < 4; h++) {
            const uint32_t w = flow_wires[f * 5 + h];
            if (w && (row_of[w] == 0 || row_of[w] == UINT32_MAX || uses[w] != 1)) return RSV_E_RANGE;
        }
    if (!out) return RSV_OK;

    Tables t;
    t.rows.assign(n_rows * ROW_WORDS, 0);
    for (size_t i = 0; i < n_rows; i++) {
        t.rows[i * ROW_WORDS] = gates[i * 6 + 3] % trace::MP;
        t.rows[i * ROW_WORDS + 2] = gates[i * 6 + 5] ? ROW_M31 : 0;
    }
    for (size_t i = 0; i < n_witness_ops; i++) {
        uint32_t* r = t.rows.data() + (size_t)witness_ops[i * 3] * ROW_WORDS;
        r[0] = witness_ops[i * 3 + 2] % trace::MP;
        r[1] = witness_ops[i * 3 + 1];
        r[2] |= ROW_WITNESS_OP;
    }
    t.flow.assign(n_flow * FLOW_WORDS, 0);
    for (size_t f = 0; f < n_flow; f++) {
        uint32_t* r = t.flow.data() + f * FLOW_WORDS;
        for (int h = 0; h < 4; h++) {
            const uint32_t w = flow_wires[f * 5 + h];
            if (!w) continue;
            const uint32_t* g = gates + (size_t)(row_of[w] - 1) * 6;
            r[2 * h] = g[0];
            r[2 * h + 1] = g[1];
            r[FLOW_MASK] |= 1u << h;
        }
        r[FLOW_SWAP_ADDR] = flow_wires[f * 5 + 4];
    }
    *out = std::move(t);
    return RSV_OK;
}

}  // namespace rsv::ucircuit
