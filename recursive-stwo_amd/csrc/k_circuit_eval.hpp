// k_circuit_eval.hpp — a caller's circuit evaluated for a batch of witnesses (rsv_circuit_eval_dev: circuit_eval_api.inc):
// `variables`, the PoseidonFlow and the swap bytes from each witness's free inputs, by the evaluation program
// circuit_eval_host.hpp compiled.  Unlike the recursion circuit's program (k_witness.hpp), whose permutation outputs are
// hints copied from the verifying pass, nobody has run a caller's permutations: they run here, inside the dependency
// order, and their records ARE the flow the trace kernels read.
//
//   k_ce_inputs  an input word >= P: atomicMin of its slot into bad[p] (k_uc_verdict, behind everything, clears ok).
//   k_ce_level   ONE level over the batch.  A workgroup is an arithmetic workgroup (blockIdx.x < arith_blocks: one lane
//                per (instruction, witness), a few dozen VALU instructions) or a Poseidon workgroup (one lane per
//                (invocation, witness), ~3 500): the branch is on blockIdx, never inside a wave.
//   k_ce_walk    the WHOLE program in one launch, a workgroup per witness: its 256 lanes share a level's instructions, then
//                its invocations, a workgroup barrier ends the level (the waves of a workgroup share the CU's L1, so what
//                one wave stored is what the next level's loads see — k_witness_small's argument).  A caller's circuit is
//                typically a chain of dependent permutations, where a launch per level is pure launch latency.
//
// Both forms run ce_exec (k_circuit_ops.hpp's circuit_op and gate_value, and the input) and ce_poseidon (the gather,
// poseidon_invoke, the output variables) and write the same words.  ce_poseidon's own: a half gathered through a link, the low
// bit of the swap variable whatever else it holds, nothing reported — k_uc_flow, run on the result, judges both.  A witness with ok[p] == 0 is not touched.  Lane order:
// with vars[variable][witness] consecutive lanes are consecutive witnesses of one instruction (a wave streams whole lines);
// with vars[witness][variable] they are consecutive instructions of one witness, whose dsts are mostly consecutive.
// A Poseidon lane: 48 B of flow table (k_uc_flow's table: user_circuit_host.hpp), its two input halves from `variables`, from a linked record or from its own record,
// the swap, the out-of-line lane-form poseidon2() (the instance k_uc_flow calls), one 128-byte record, the swap byte, and
// up to four output variables; 16-byte loads and stores, the state in registers.
#pragma once
#include "circuit_eval_host.hpp"
#include "k_circuit_ops.hpp"
#include "k_user_circuit.hpp"

namespace rsv {

struct CeArgs {
    const uint4* instr;       // [n_instr][2]
    const uint32_t* levels;   // [n_levels + 1] into instr
    const uint32_t* flevels;  // [n_levels + 1] into forder
    const uint32_t* forder;   // [n_flow]: the invocations, level after level
    const uint4* src;         // [n_flow][3]: the flow table (user_circuit_host.hpp)
    uint32_t n_levels, n_flow, n_vars, n_inputs, n;
    bool by_variable;
    const uint4* inputs;      // [n][n_inputs]
    uint4* vars;              // [n][n_vars] (by_variable = 0) or [n_vars][n]
    uint4* flow;              // [n][n_flow][8]
    uint8_t* swap;            // [n][n_flow]
    const uint8_t* ok;        // [n]: 0 = the witness is skipped
    uint32_t ibegin, iend, fbegin, fend, arith_blocks;  // k_ce_level: this level's instructions and invocations
};

__device__ __forceinline__ uint32_t ce_word(uint32_t w) { return w < P ? w : 0u; }

// one instruction for one witness: the shared ops, and this program's own two
__device__ __forceinline__ void ce_exec(const CeArgs& a, uint32_t i, uint32_t p) {
    const uint4 w0 = a.instr[(size_t)i * 2], w1 = a.instr[(size_t)i * 2 + 1];
    const auto var = [&](uint32_t w) -> uint4& { return var_at(a.vars, a.by_variable, a.n, a.n_vars, p, w); };
    var(w0.y) = circuit_op(w0, w1, var, [&]() {
        if (w0.x == ceval::E_GATE) return u4_of(gate_value(var(w0.z), var(w0.w), w1.x, w1.z != 0, w1.y, var));
        if (w0.x != ceval::E_INPUT) return make_uint4(0, 0, 0, 0);
        const uint4 v = a.inputs[(size_t)p * a.n_inputs + w1.x];  // a word at or above P has been reported by k_ce_inputs; it counts as 0
        return make_uint4(ce_word(v.x), ce_word(v.y), ce_word(v.z), ce_word(v.w));
    });
}

// invocation k of witness p
__device__ __forceinline__ void ce_poseidon(const CeArgs& a, uint32_t k, uint32_t p) {
    const uint4 s0 = a.src[(size_t)k * 3], s1 = a.src[(size_t)k * 3 + 1], s2 = a.src[(size_t)k * 3 + 2];
    const uint32_t wire[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, link[2] = {s2.z, s2.w}, mask = s2.x, addr = s2.y;
    const size_t rec = (size_t)p * a.n_flow + k;
    uint4* f = a.flow + rec * 8;
    const auto var = [&](uint32_t w) -> uint4& { return var_at(a.vars, a.by_variable, a.n, a.n_vars, p, w); };
    uint4 in[4];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if ((mask >> h) & 1u) {
            in[2 * h] = var(wire[2 * h]);
            in[2 * h + 1] = var(wire[2 * h + 1]);
        } else {  // a linked invocation's output half, else the caller's words in this record
            const uint4* from = link[h] ? a.flow + ((size_t)p * a.n_flow + (link[h] - 1) / 2) * 8 + 4 + 2 * ((link[h] - 1) & 1u) : f + 2 * h;
            in[2 * h] = from[0];
            in[2 * h + 1] = from[1];
        }
    }
    // any value's low bit swaps, and non-canonical words are not reported here: k_uc_flow, run on the result, does both
    poseidon_invoke(in, addr ? var(addr).x & 1u : 0u, true, f, a.swap + rec, [&](int q, uint4 o) {
        if ((mask >> (ucircuit::FLOW_DEFINES + q)) & 1u) var(wire[4 + q]) = o;
    });
}

__global__ __launch_bounds__(256) void k_ce_inputs(const uint4* __restrict__ inputs, uint32_t n_inputs, uint32_t n,
                                                   const uint8_t* __restrict__ ok, uint32_t* __restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n * n_inputs) return;
    const uint32_t p = (uint32_t)(t / n_inputs), slot = (uint32_t)(t % n_inputs);
    if (ok[p] && !uc_canonical(inputs[t])) atomicMin(bad + p, slot);
}

// lane t of a level's `count` items over n witnesses -> (item, witness), in the order the layout streams
__device__ __forceinline__ bool ce_lane(const CeArgs& a, uint64_t t, uint32_t count, uint32_t& item, uint32_t& p) {
    if (t >= (uint64_t)count * a.n) return false;
    if (a.by_variable) { item = (uint32_t)(t / a.n); p = (uint32_t)(t % a.n); }
    else { p = (uint32_t)(t / count); item = (uint32_t)(t % count); }
    return a.ok[p] != 0;
}

__global__ __launch_bounds__(256) void k_ce_level(CeArgs a) {
    uint32_t item, p;
    if (blockIdx.x < a.arith_blocks) {
        if (!ce_lane(a, (uint64_t)blockIdx.x * 256 + threadIdx.x, a.iend - a.ibegin, item, p)) return;
        ce_exec(a, a.ibegin + item, p);
    } else {
        if (!ce_lane(a, (uint64_t)(blockIdx.x - a.arith_blocks) * 256 + threadIdx.x, a.fend - a.fbegin, item, p)) return;
        ce_poseidon(a, a.forder[a.fbegin + item], p);
    }
}

// Workgroup p walks every level for witness p.  The barrier is in workgroup-uniform control flow: a skipped witness's
// workgroup leaves as a whole before the first one, and the loop bounds are the program's.
__global__ __launch_bounds__(256) void k_ce_walk(CeArgs a) {
    const uint32_t p = blockIdx.x;
    if (!a.ok[p]) return;
    for (uint32_t l = 0; l < a.n_levels; l++) {
        for (uint32_t i = a.levels[l] + threadIdx.x, end = a.levels[l + 1]; i < end; i += 256) ce_exec(a, i, p);
        for (uint32_t j = a.flevels[l] + threadIdx.x, end = a.flevels[l + 1]; j < end; j += 256) ce_poseidon(a, a.forder[j], p);
        __threadfence_block();
        __syncthreads();
    }
}

}  // namespace rsv
