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
// Both forms run ce_exec and ce_poseidon and write the same words.  A witness with ok[p] == 0 is not touched.  Lane order:
// with vars[variable][witness] consecutive lanes are consecutive witnesses of one instruction (a wave streams whole lines);
// with vars[witness][variable] they are consecutive instructions of one witness, whose dsts are mostly consecutive.
// A Poseidon lane: 48 B of flow table, its two input halves from `variables`, from a linked record or from its own record,
// the swap, the out-of-line lane-form poseidon2() (the instance k_uc_flow calls), one 128-byte record, the swap byte, and
// up to four output variables; 16-byte loads and stores, the state in registers.
#pragma once
#include "circuit_eval_host.hpp"
#include "k_user_circuit.hpp"
#include "k_witness.hpp"

namespace rsv {

static_assert(ceval::E_CONST == W_CONST && ceval::E_ADD == W_ADD && ceval::E_MUL == W_MUL && ceval::E_MULC == W_MULC &&
                  ceval::E_COPY == W_COPY && ceval::E_INV == W_INV && ceval::E_INV0 == W_INV0 && ceval::E_QINV == W_QINV &&
                  ceval::E_CINV == W_CINV && ceval::E_COORD == W_COORD && ceval::E_BIT == W_BIT && ceval::E_INPUT >= W_N_OPS,
              "circuit_eval_host.hpp and layout.hpp disagree");

struct CeArgs {
    const uint4* instr;       // [n_instr][2]
    const uint32_t* levels;   // [n_levels + 1] into instr
    const uint32_t* flevels;  // [n_levels + 1] into forder
    const uint32_t* forder;   // [n_flow]: the invocations, level after level
    const uint4* src;         // [n_flow][3]: ceval's flow table
    uint32_t n_levels, n_flow, n_vars, n_inputs, n;
    bool by_variable;
    const uint4* inputs;      // [n][n_inputs]
    uint4* vars;              // [n][n_vars] (by_variable = 0) or [n_vars][n]
    uint4* flow;              // [n][n_flow][8]
    uint8_t* swap;            // [n][n_flow]
    const uint8_t* ok;        // [n]: 0 = the witness is skipped
    uint32_t ibegin, iend, fbegin, fend, arith_blocks;  // k_ce_level: this level's instructions and invocations
};

__device__ __forceinline__ uint4& ce_var(const CeArgs& a, uint32_t p, uint32_t w) {
    return a.by_variable ? a.vars[(size_t)w * a.n + p] : a.vars[(size_t)p * a.n_vars + w];
}
__device__ __forceinline__ uint32_t ce_word(uint32_t w) { return w < P ? w : 0u; }

// one instruction for one witness: the hint ops as witness_exec has them, the input and the general gate
__device__ __forceinline__ void ce_exec(const CeArgs& a, const uint4 w0, const uint4 w1, uint32_t p) {
    const uint32_t op = w0.x, dst = w0.y, x = w0.z, y = w0.w, i0 = w1.x;
    uint4 r = make_uint4(0, 0, 0, 0);
    switch (op) {
    case W_CONST: r = w1; break;
    case W_ADD: r = u4_of(q_add(q_of(ce_var(a, p, x)), q_of(ce_var(a, p, y)))); break;
    case W_MUL: r = u4_of(q_mul(q_of(ce_var(a, p, x)), q_of(ce_var(a, p, y)))); break;
    case W_MULC: r = u4_of(q_mul_m(q_of(ce_var(a, p, x)), i0)); break;
    case W_COPY: r = ce_var(a, p, x); break;
    case W_INV: r.x = m_inv(ce_var(a, p, x).x); break;  // 0 -> 0
    case W_INV0: r.x = m_inv(ce_var(a, p, x).x); break;
    case W_QINV: {
        const uint4 v = ce_var(a, p, x);
        if (v.x | v.y | v.z | v.w) r = u4_of(q_inv(q_of(v)));
        break;
    }
    case W_CINV: {
        const uint4 v = ce_var(a, p, x);
        if (v.x | v.y) {
            const CM31 c = c_inv(c_mk(v.x, v.y));
            r.x = i0 ? c.b : c.a;
        }
        break;
    }
    case W_COORD: {
        const uint4 v = ce_var(a, p, x);
        r.x = i0 == 0 ? v.x : i0 == 1 ? v.y : i0 == 2 ? v.z : v.w;
        break;
    }
    case W_BIT: r.x = (ce_var(a, p, x).x >> i0) & 1u; break;
    case ceval::E_INPUT: {  // a word at or above P has been reported by k_ce_inputs; it counts as 0
        const uint4 v = a.inputs[(size_t)p * a.n_inputs + i0];
        r = make_uint4(ce_word(v.x), ce_word(v.y), ce_word(v.z), ce_word(v.w));
        break;
    }
    case ceval::E_GATE: {  // op (a + b) + (1 - op) a b
        uint32_t k = i0;
        if (w1.z) k = ce_var(a, p, w1.y).x ? i0 : 0u;
        const QM31 qa = q_of(ce_var(a, p, x)), qb = q_of(ce_var(a, p, y));
        r = u4_of(q_add(q_mul_m(q_add(qa, qb), k), q_mul_m(q_mul(qa, qb), m_sub(1u, k))));
        break;
    }
    default: break;
    }
    ce_var(a, p, dst) = r;
}
__device__ __forceinline__ void ce_exec(const CeArgs& a, uint32_t i, uint32_t p) { ce_exec(a, a.instr[(size_t)i * 2], a.instr[(size_t)i * 2 + 1], p); }

// invocation k of witness p
__device__ __forceinline__ void ce_poseidon(const CeArgs& a, uint32_t k, uint32_t p) {
    const uint4 s0 = a.src[(size_t)k * 3], s1 = a.src[(size_t)k * 3 + 1], s2 = a.src[(size_t)k * 3 + 2];
    const uint32_t wire[4] = {s0.x, s0.y, s0.z, s0.w}, out_var[4] = {s1.x, s1.y, s1.z, s1.w}, link[2] = {s2.z, s2.w};
    const uint32_t mask = s2.x, addr = s2.y;
    const size_t rec = (size_t)p * a.n_flow + k;
    uint4* f = a.flow + rec * 8;
    uint4 in[4];
    bool good = true;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if ((mask >> h) & 1u) {
            in[2 * h] = ce_var(a, p, wire[2 * h]);
            in[2 * h + 1] = ce_var(a, p, wire[2 * h + 1]);
        } else {  // a linked invocation's output half, else the caller's words in this record
            const uint4* from = link[h] ? a.flow + ((size_t)p * a.n_flow + (link[h] - 1) / 2) * 8 + 4 + 2 * ((link[h] - 1) & 1u) : f + 2 * h;
            in[2 * h] = from[0];
            in[2 * h + 1] = from[1];
        }
        good = good && uc_canonical(in[2 * h]) && uc_canonical(in[2 * h + 1]);
    }
    const uint32_t sw = addr ? ce_var(a, p, addr).x & 1u : 0u;
    State16 st;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint4 v = sw ? in[(q + 2) & 3] : in[q];
        if (!good) v = make_uint4(0, 0, 0, 0);  // the permutation takes canonical words only (as k_uc_flow, which then reports the invocation)
        st.s[4 * q] = v.x; st.s[4 * q + 1] = v.y; st.s[4 * q + 2] = v.z; st.s[4 * q + 3] = v.w;
    }
    st = poseidon2(st);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 o = make_uint4(st.s[4 * q], st.s[4 * q + 1], st.s[4 * q + 2], st.s[4 * q + 3]);
        f[q] = in[q];
        f[4 + q] = o;
        if (out_var[q]) ce_var(a, p, out_var[q]) = o;
    }
    a.swap[rec] = (uint8_t)sw;
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
