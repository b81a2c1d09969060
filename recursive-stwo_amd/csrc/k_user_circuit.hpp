// k_user_circuit.hpp — the reference's two pre-prove checks for a batch of witnesses of ONE circuit that lie in HBM
// (rsv_circuit_check_dev, rsv_circuit_flow_dev: user_circuit_api.inc), for any program with a gate list.
//
//   k_uc_gates   cs.check_arithmetics() (constraint_system/src/plonk_with_poseidon.rs:337-381): for every row
//                c == op (a + b) + (1 - op) a b in QM31, c an M31 where enforce_c_m31 is set.
//   k_uc_flow    cs.check_poseidon_invocations() (:468-519), which at the same time MAKES the PoseidonFlow the trace
//                kernels read: the wire-bound halves are gathered from `variables`, the permutation's output is written.
//   k_uc_verdict ok[p] = 0 where a row or an invocation failed.
//
// Neither check kernel writes ok: a lane that cleared it would make the lanes of the same proof that start later skip
// their rows, and bad[p] would no longer be the smallest failing index.  They only atomicMin into bad[p] (preset to all
// ones by the driver); k_uc_verdict, behind them on the stream, clears ok.  No lane waits for another.
//
// MI355X mapping.  k_uc_gates is the read side of k_trace_plonk: one lane per (row, proof), a workgroup's 256 rows belong
// to one proof, 16 B of row table + 12 B of wires (shape constants, L2 resident) and three 16-byte gathers into the proof's
// vector per lane, ~40 multiplies, no store but the rare atomic.  Padding rows are not visited.  k_uc_flow: one lane per
// (invocation, proof), a wave's 64 invocations belong to one proof; 48 B of source table, up to eight 16-byte gathers,
// one out-of-line permutation (poseidon2(), the lane form: the state in registers), one 128-byte record.
// The gate formula (gate_value) and the invocation (poseidon_invoke) are k_circuit_ops.hpp's, shared with k_circuit_eval.hpp,
// and so is the flow table (user_circuit_host.hpp; k_uc_flow reads neither its define bits nor its links).  k_uc_flow's own:
// the swap variable has to be the QM31 0 or 1, a bound output is compared with its pair, the failing invocation is reported.
#pragma once
#include "k_circuit_ops.hpp"
#include "k_trace.hpp"
#include "user_circuit_host.hpp"

namespace rsv {

struct UcArgs {
    const uint4* vars;          // [n][n_vars] (by_variable = 0) or [n_vars][n] QM31
    uint32_t n_vars, n;
    bool by_variable;
    const uint8_t* ok;          // [n]: 0 = the proof is skipped
    uint32_t* bad;              // [n]: preset to 0xffffffff; atomicMin of the failing rows / invocations
    const uint32_t* wires;      // [3][2^lp] padded a / b / c wires
    uint32_t log_plonk;
    const uint4* rows;          // [n_rows]: op (or the witness op's constant), bit variable, flags, 0
    uint32_t n_rows;
    const uint4* src;           // [n_flow][3]: the flow source table
    uint32_t n_flow;
    uint4* flow;                // [n][n_flow][8]: r1, r2 (in for a half without a wire, else out), r3, r4 (out)
    uint8_t* swap;              // [n][n_flow] (out)
};

// Block b: proof b / per, rows (b % per) * 256 ..., per = ceil(n_rows / 256).
__global__ __launch_bounds__(256) void k_uc_gates(UcArgs a) {
    const uint32_t per = (a.n_rows + 255) / 256;
    const uint32_t p = blockIdx.x / per, row = (blockIdx.x % per) * 256 + threadIdx.x;
    if (p >= a.n || row >= a.n_rows || !a.ok[p]) return;
    const size_t N = (size_t)1 << a.log_plonk;
    const uint4 t = a.rows[row];
    const auto var = [&](uint32_t w) { return var_at(a.vars, a.by_variable, a.n, a.n_vars, p, w); };
    const uint4 va = var(a.wires[row]), vb = var(a.wires[N + row]), vc = var(a.wires[2 * N + row]);
    bool good = uc_canonical(va) && uc_canonical(vb) && uc_canonical(vc);
    // words at or above P have failed already, what they give here is dropped (computed whatever `good` is: no load waits for a verdict)
    const QM31 want = gate_value(va, vb, t.x, t.z & ucircuit::ROW_WITNESS_OP, t.y, var);
    good = good && q_eq(want, q_of(vc));
    if (t.z & ucircuit::ROW_M31) good = good && (vc.y | vc.z | vc.w) == 0;
    if (row < 4) good = good && va.x == (row == 1) && va.y == (row == 2) && va.z == (row == 3) && va.w == 0;  // variables 0..3 = 0, 1, i, j
    if (!good) atomicMin(a.bad + p, row);
}

// Block b (one wave): proof b / per, invocations (b % per) * 64 ..., per = ceil(n_flow / 64).
__global__ __launch_bounds__(64) void k_uc_flow(UcArgs a) {
    const uint32_t per = (a.n_flow + TRACE_WAVE - 1) / TRACE_WAVE;
    const uint32_t p = blockIdx.x / per, k = (blockIdx.x % per) * TRACE_WAVE + threadIdx.x;
    if (p >= a.n || k >= a.n_flow) return;
    const size_t rec = (size_t)p * a.n_flow + k;
    uint4* f = a.flow + rec * 8;
    if (!a.ok[p]) {  // a skipped proof: zero records (uniform: one proof per workgroup)
#pragma unroll
        for (int q = 0; q < 8; q++) f[q] = make_uint4(0, 0, 0, 0);
        a.swap[rec] = 0;
        return;
    }
    const uint4 s0 = a.src[(size_t)k * 3], s1 = a.src[(size_t)k * 3 + 1], s2 = a.src[(size_t)k * 3 + 2];
    const uint32_t wire[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, mask = s2.x, addr = s2.y;
    const auto var = [&](uint32_t w) { return var_at(a.vars, a.by_variable, a.n, a.n_vars, p, w); };
    uint4 in[4];  // r1, r2 as given: from `variables` where the half has a wire, else from the record
#pragma unroll
    for (int q = 0; q < 4; q++) in[q] = (mask >> (q >> 1)) & 1u ? var(wire[q]) : f[q];
    bool good = true;
    uint32_t sw = 0;
    if (addr) {  // the swap bit has to be the QM31 0 or 1
        const uint4 b = var(addr);
        good = b.x <= 1u && (b.y | b.z | b.w) == 0;
        sw = b.x & 1u;
    }
    bool bound = true;  // a bound output is its pair in `variables`
    good = poseidon_invoke(in, sw, good, f, a.swap + rec, [&](int q, uint4 o) {
        if (!((mask >> (2 + (q >> 1))) & 1u)) return;
        const uint4 v = var(wire[4 + q]);
        bound = bound && v.x == o.x && v.y == o.y && v.z == o.z && v.w == o.w;
    });
    if (!(good && bound)) atomicMin(a.bad + p, k);
}

__global__ __launch_bounds__(256) void k_uc_verdict(const uint32_t* __restrict__ bad, uint32_t n, uint8_t* __restrict__ ok) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p < n && bad[p] != 0xffffffffu) ok[p] = 0;
}

}  // namespace rsv
