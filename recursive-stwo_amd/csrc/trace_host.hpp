// trace_host.hpp — HOST code, plain C++ (no HIP): the log sizes and the PREPROCESSED columns of the recursion circuit's two
// components, from the shape's gate list and flow wires (rsv_trace_log_sizes / rsv_trace_preprocessed, include/rsv.h).
// The trace columns, which depend on the proof, are the device's (k_trace.hpp).  Included by trace_api.inc; compiles on
// its own with g++ (round constants are passed in), so a sanitizer build can drive it without a device.
//
//   pad()                      constraint_system/src/plonk_with_poseidon.rs:283-331
//   populate_logup_arguments   :345-466 (multiplicities of the three wire lookups and of the Poseidon wires)
//   Plonk preprocessed order   components/recursive/composition/src/plonk.rs:14-41
//   Poseidon preprocessed      components/recursive/composition/src/poseidon.rs:73-241 (six rows per invocation)
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rsv.h"

namespace rsv::trace {

constexpr uint32_t MP = 0x7fffffffu;
constexpr uint32_t PLONK_PRE_COLS = 10, POSEIDON_PRE_COLS = 40, PLONK_TRACE_COLS = 12, POSEIDON_TRACE_COLS = 48;
// The preprocessed columns the logup relations read (k_interaction.hpp), by their index in preprocessed()'s tables; op,
// enforce_c_m31, is_full, rc0[1..15] and rc1 are read by no relation.
constexpr uint32_t PLONK_A_WIRE = 0, PLONK_B_WIRE = 1, PLONK_C_WIRE = 2, PLONK_MULT_A = 4, PLONK_MULT_B = 5, PLONK_MULT_C = 6,
                   PLONK_POSEIDON_WIRE = 7, PLONK_MULT_POSEIDON = 8;
constexpr uint32_t POSEIDON_IS_FIRST = 0, POSEIDON_IS_LAST = 1, POSEIDON_ROUND_ID = 3, POSEIDON_SWAP_ADDR = 4 /* rc0[0] */,
                   POSEIDON_EXT_WIRE_1 = 36, POSEIDON_EXT_WIRE_2 = 37, POSEIDON_EXT_NZ_1 = 38, POSEIDON_EXT_NZ_2 = 39;
constexpr uint32_t ROWS_PER_INVOCATION = 6;
// The constraint system starts with four constant variables (0, 1, i, j) and one row each (plonk_with_poseidon.rs:95-
// 137); num_input counts the three non-zero ones and every new_*(PublicInput) after them: the public inputs are
// variables 1 .. num_input.  components/recursive allocates no public input (only components/last calls
// new_public_input), so the recursion circuit's num_input is 3, which rsv_trace_preprocessed passes.
constexpr uint32_t NUM_INPUT = 3;
constexpr uint32_t MAX_WIRE = 1u << 26;  // rsv_witness_program_create's bound on n_vars

inline uint32_t ceil_log2(uint64_t x) {
    uint32_t l = 0;
    while ((1ull << l) < x) l++;
    return l;
}

// Invocations after pad(): a multiple of 16, at least 32.
inline uint64_t padded_flow(uint64_t n_flow) {
    const uint64_t r = (n_flow + 15) / 16 * 16;
    return r < 32 ? 32 : r;
}

// log_plonk = next_power_of_two of the row count (pad()).  log_poseidon: the Poseidon trace generator sits in stwo's
// fork, which the reference does not vendor; ceil_log2(6 * padded invocations) reproduces the header of the next
// fixture for all 14 consecutive pairs of the reference's chain (tests/golden/recursion_circuit_pins.json).
inline int log_sizes(uint64_t n_rows, uint64_t n_flow, uint32_t& log_plonk, uint32_t& log_poseidon) {
    if (n_rows == 0 || n_flow == 0) return RSV_E_SIZE;
    const uint32_t lp = ceil_log2(n_rows), lq = ceil_log2(ROWS_PER_INVOCATION * padded_flow(n_flow));
    if (lp > RSV_MAX_WITNESS_LOG || lq > RSV_MAX_WITNESS_LOG) return RSV_E_SIZE;
    log_plonk = lp;
    log_poseidon = lq;
    return RSV_OK;
}

// The padded a / b / c wires, [3][2^log_plonk]: padding rows are (0, 0, 0) (pad(): cs._row(0, 0, 0, 1)).
inline std::vector<uint32_t> padded_wires(const uint32_t* gates, size_t n_rows, uint32_t log_plonk) {
    const size_t N = (size_t)1 << log_plonk;
    std::vector<uint32_t> w(3 * N, 0);
    for (size_t i = 0; i < n_rows; i++)
        for (int k = 0; k < 3; k++) w[k * N + i] = gates[i * 6 + k];
    return w;
}

// gates [n_rows][6] = a, b, c, op, poseidon_wire, enforce_c_m31; flow_wires [n_flow][5] = wires of r1..r4, swap address;
// num_input: see NUM_INPUT (RSV_E_RANGE below 3 or beyond the variables the arrays name); round constants: first [4][16],
// partial [14], last [4][16].  plonk_pre [10][2^log_plonk], poseidon_pre [40][2^log_poseidon].
// Everything is checked before anything is written: on an error status the outputs are untouched.
inline int preprocessed(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, uint32_t log_plonk,
                        uint32_t log_poseidon, uint32_t num_input, const uint32_t (*rc_first)[16], const uint32_t* rc_partial, const uint32_t (*rc_last)[16],
                        uint32_t* plonk_pre, uint32_t* poseidon_pre) {
    if (!gates || !flow_wires || !plonk_pre || !poseidon_pre || !rc_first || !rc_partial || !rc_last) return RSV_E_NULL;
    uint32_t need_lp = 0, need_lq = 0;
    int rc = log_sizes(n_rows, n_flow, need_lp, need_lq);
    if (rc != RSV_OK) return rc;
    if (log_plonk < need_lp || log_poseidon < need_lq || log_plonk > RSV_MAX_WITNESS_LOG || log_poseidon > RSV_MAX_WITNESS_LOG)
        return RSV_E_SIZE;
    if (n_rows < 4) return RSV_E_RANGE;
    if (num_input < NUM_INPUT || num_input >= MAX_WIRE) return RSV_E_RANGE;
    for (uint32_t k = 0; k < 4; k++) {  // the four constant rows (k, 0, k, op 1)
        const uint32_t* g = gates + (size_t)k * 6;
        if (g[0] != k || g[1] != 0 || g[2] != k || g[3] != 1 || g[4] != 0 || g[5] != 0) return RSV_E_RANGE;
    }
    uint32_t n_vars = num_input + 1;
    for (size_t i = 0; i < n_rows; i++)
        for (int k : {0, 1, 2, 4}) {
            const uint32_t w = gates[i * 6 + k];
            if (w >= MAX_WIRE) return RSV_E_RANGE;
            if (w >= n_vars) n_vars = w + 1;
        }
    for (size_t i = 0; i < n_flow * 5; i++) {
        if (flow_wires[i] >= MAX_WIRE) return RSV_E_RANGE;
        if (flow_wires[i] >= n_vars) n_vars = flow_wires[i] + 1;
    }
    const size_t N = (size_t)1 << log_plonk, Q = (size_t)1 << log_poseidon, n_pad = padded_flow(n_flow);

    // populate_logup_arguments (:345-466) over the padded rows and flow.  Padding rows read wire 0 three times, padding
    // invocations have swap address 0.
    std::vector<int64_t> counts(n_vars, 0), mp_vars(n_vars, 0);
    for (size_t i = 0; i < n_rows; i++)
        for (int k = 0; k < 3; k++) counts[gates[i * 6 + k]]++;
    counts[0] += 3 * (int64_t)(N - n_rows);
    for (uint32_t k = 1; k <= num_input; k++) counts[k]++;
    for (size_t f = 0; f < n_flow; f++) counts[flow_wires[f * 5 + 4]]++;
    counts[0] += (int64_t)(n_pad - n_flow);
    std::vector<uint32_t> mult(3 * N, 1);  // mult_a, mult_b, mult_c: 1, except 1 - count at a variable's first use
    std::vector<uint8_t> seen(n_vars, 0);
    auto mod = [](int64_t v) { return (uint32_t)(((v % (int64_t)MP) + MP) % MP); };
    for (size_t i = 0; i < N; i++)
        for (int k = 0; k < 3; k++) {
            const uint32_t w = i < n_rows ? gates[i * 6 + k] : 0;
            if (!seen[w]) {
                seen[w] = 1;
                mult[k * N + i] = mod(1 - counts[w]);
            }
        }
    for (size_t f = 0; f < n_flow; f++)
        for (int j = 0; j < 4; j++) mp_vars[flow_wires[f * 5 + j]]++;
    mp_vars[0] = 0;
    std::vector<uint32_t> mult_poseidon(N, 0);
    for (size_t i = 0; i < n_rows; i++) {
        const uint32_t w = gates[i * 6 + 4];
        if (mp_vars[w]) {
            if (counts[w] != 1) return RSV_E_RANGE;  // a Poseidon output is used once (the reference asserts it)
            mult_poseidon[i] = (uint32_t)(mp_vars[w] % MP);
            mp_vars[w] = 0;
        }
    }

    // Plonk: a_wire, b_wire, c_wire, op, mult_a, mult_b, mult_c, poseidon_wire, mult_poseidon, enforce_c_m31
    auto pcol = [&](int c) { return plonk_pre + (size_t)c * N; };
    std::memset(plonk_pre, 0, PLONK_PRE_COLS * N * 4);
    for (size_t i = 0; i < n_rows; i++) {
        const uint32_t* g = gates + i * 6;
        pcol(0)[i] = g[0];
        pcol(1)[i] = g[1];
        pcol(2)[i] = g[2];
        pcol(3)[i] = g[3] % MP;
        pcol(7)[i] = g[4];
        pcol(9)[i] = g[5] % MP;
    }
    for (size_t i = n_rows; i < N; i++) pcol(3)[i] = 1;
    std::memcpy(pcol(4), mult.data(), 3 * N * 4);
    std::memcpy(pcol(8), mult_poseidon.data(), N * 4);

    // Poseidon: is_first, is_last, is_full, round_id, rc0[16], rc1[16], wire r1..r4 on the first / last row, wire != 0
    auto qcol = [&](int c) { return poseidon_pre + (size_t)c * Q; };
    std::memset(poseidon_pre, 0, POSEIDON_PRE_COLS * Q * 4);
    for (size_t k = 0; k < n_pad; k++) {
        const uint32_t* fw = k < n_flow ? flow_wires + k * 5 : nullptr;
        const uint32_t w1 = fw ? fw[0] : 0, w2 = fw ? fw[1] : 0, w3 = fw ? fw[2] : 0, w4 = fw ? fw[3] : 0, addr = fw ? fw[4] : 0;
        size_t row[6];
        for (size_t j = 0; j < 6; j++) row[j] = ((k / 16) * 6 + j) * 16 + k % 16;
        for (size_t j = 0; j < 6; j++) qcol(3)[row[j]] = (uint32_t)((6 * k + j) % MP);
        qcol(0)[row[0]] = 1;
        qcol(1)[row[5]] = 1;
        for (int j : {1, 2, 4, 5}) qcol(2)[row[j]] = 1;
        qcol(4)[row[0]] = addr;  // rc0[0] of the first row carries the swap bit's address
        const uint32_t (*pairs[4])[16] = {rc_first, rc_first + 2, rc_last, rc_last + 2};
        const int prow[4] = {1, 2, 4, 5};
        for (int t = 0; t < 4; t++)
            for (int i = 0; i < 16; i++) {
                qcol(4 + i)[row[prow[t]]] = pairs[t][0][i];
                qcol(20 + i)[row[prow[t]]] = pairs[t][1][i];
            }
        for (int r = 0; r < 14; r++) qcol(4 + r)[row[3]] = rc_partial[r];
        qcol(36)[row[0]] = w1; qcol(37)[row[0]] = w2; qcol(38)[row[0]] = w1 != 0; qcol(39)[row[0]] = w2 != 0;
        qcol(36)[row[5]] = w3; qcol(37)[row[5]] = w4; qcol(38)[row[5]] = w3 != 0; qcol(39)[row[5]] = w4 != 0;
    }
    for (size_t r = ROWS_PER_INVOCATION * n_pad; r < Q; r++) qcol(0)[r] = qcol(1)[r] = 1;  // first and last round at once
    return RSV_OK;
}

}  // namespace rsv::trace
