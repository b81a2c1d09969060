// k_trace.hpp — the TRACE columns of the recursion circuit's two components for a batch of proofs
// (rsv_witness_trace_dev, trace_api.inc), from what rsv_witness_eval_dev left in HBM: `variables` and the PoseidonFlow.
//
//   Plonk      12 columns a_val, b_val, c_val (4 words each) = variables[wire[row]]
//              (constraint_system/src/plonk_with_poseidon.rs:571-618), 2^lp rows after pad().
//   Poseidon   48 columns in[16], intermediate[16], out[16], six rows per invocation
//              (components/recursive/composition/src/poseidon.rs:73-241): the state at every round boundary, the
//              full-round S-box outputs and the 14 partial-round S-box outputs; invocation k sits at rows
//              ((k / 16) * 6 + j) * 16 + k % 16, j < 6 (blocks of 96 rows for 16 invocations); rows behind the padded
//              flow are zero.
//
// MI355X mapping: both are HBM-write streams (12 x 4 B per Plonk row, 1 152 B per invocation).
// k_trace_plonk: one lane per (row, proof); the wires are shape constants every proof reads (L2 / MALL resident), the
// 16-byte gathers of `variables` hit a proof's 0.8 - 5 MB vector, and consecutive workgroups take consecutive rows of ONE
// proof so that the workgroups in flight share a handful of proofs.  Stores: 12 dwords per lane, coalesced per column.
// k_trace_poseidon: one lane per invocation, the state in registers (plain canonical arithmetic: the write, not the
// permutation, is the cost).  A wave owns 64 aligned invocations = 384 contiguous rows of every column.  Rows j and j + 1
// of one 16-invocation block form one 128-byte line per column, so the wave stages a pair of rows (16 columns at a
// time, 8 KB of LDS) and stores whole lines: eight lanes per line, 16 B each (k_emulated.hpp measured 2.4 TB/s for
// piecewise line writes against 5.6 TB/s for whole lines).
#pragma once
#include "poseidon2.hpp"

namespace rsv {

constexpr uint32_t PLONK_COLS_K = 12, POSEIDON_COLS_K = 48;

struct TraceArgs {
    static constexpr bool hashed = false;  // (TraceStmtArgs)
    const uint4* vars;          // [n][n_vars] (by_variable = 0) or [n_vars][n] QM31
    uint32_t n_vars, n;
    bool by_variable;
    const uint8_t* accept;      // [n]
    const uint32_t* wires;      // [3][2^lp] padded a / b / c wires
    uint32_t log_plonk;
    uint32_t* plonk;            // [n][12][2^lp]
    const uint4* flow;          // [n][flow_count][8]: r1, r2, r3, r4 (8 words each)
    const uint8_t* swap;        // [n][flow_count]
    uint32_t flow_count, copies;
    uint32_t n_pad;             // invocations after pad(): multiple of 16, >= 32
    uint32_t log_poseidon;
    uint32_t* poseidon;         // [n][48][2^lq]
};

// A hashed program (rsv_witness_program_build_inputs_hashed): the invocations behind the copies', k = copies * flow_count ..
// + stmt_flow, are the statement hash's, whose records lie at the tail of the flow buffers: [n][stmt_flow] from record `tail`.
struct TraceStmtArgs : TraceArgs {
    static constexpr bool hashed = true;
    uint32_t stmt_flow;
    size_t tail;
};

// ---------------------------------------------------------------- Plonk
// Block b: proof b / blocks_per_proof, rows (b % blocks_per_proof) * 256 ...: the workgroups in flight share proofs.
__global__ __launch_bounds__(256) void k_trace_plonk(TraceArgs a) {
    const uint32_t N = 1u << a.log_plonk, per = (N + 255) / 256;
    const uint32_t p = blockIdx.x / per, row = (blockIdx.x % per) * 256 + threadIdx.x;
    if (p >= a.n || row >= N) return;
    const bool ok = a.accept[p] != 0;
    uint32_t* out = a.plonk + (size_t)p * PLONK_COLS_K * N + row;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) {
            const uint32_t w = a.wires[(size_t)k * N + row];
            v = a.by_variable ? a.vars[(size_t)w * a.n + p] : a.vars[(size_t)p * a.n_vars + w];
        }
        out[(size_t)(4 * k + 0) * N] = v.x;
        out[(size_t)(4 * k + 1) * N] = v.y;
        out[(size_t)(4 * k + 2) * N] = v.z;
        out[(size_t)(4 * k + 3) * N] = v.w;
    }
}

// d_ops[p][k] = op of witness-op row k for proof p: variables[bit].x ? constant : 0 (CirclePointM31Var::select,
// primitives/circle/src/lib.rs:83-98); zero for a rejected proof.
__global__ __launch_bounds__(256) void k_trace_ops(TraceArgs a, const uint32_t* __restrict__ wops, uint32_t n_ops, uint32_t* __restrict__ ops) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n_ops * a.n) return;
    const uint32_t p = (uint32_t)(t / n_ops), k = (uint32_t)(t % n_ops);
    uint32_t v = 0;
    if (a.accept[p]) {
        const uint32_t bit = wops[3 * k + 1];
        const uint32_t x = a.by_variable ? a.vars[(size_t)bit * a.n + p].x : a.vars[(size_t)p * a.n_vars + bit].x;
        v = x ? wops[3 * k + 2] : 0u;
    }
    ops[t] = v;
}

// ---------------------------------------------------------------- Poseidon
__device__ __forceinline__ void trace_ext(uint32_t* s) { mds16_ref(s); }

// One full round pair (two rounds): mid = S-box outputs of the first round, s -> the state after both.
__device__ __forceinline__ void trace_full_pair(uint32_t* s, uint32_t* mid, int r) {
#pragma unroll
    for (int i = 0; i < 16; i++) mid[i] = pow5_ref(m_add(s[i], RC_FULL[r][i]));
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = mid[i];
    trace_ext(s);
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = pow5_ref(m_add(s[i], RC_FULL[r + 1][i]));
    trace_ext(s);
}

constexpr uint32_t TRACE_WAVE = 64;
constexpr uint32_t TRACE_STAGE = 16 * 2 * TRACE_WAVE;  // 16 columns x 2 rows x 64 invocations (8 KB)

// Columns c0 .. c0 + 15 of rows (j, j + 1) of the wave's 64 invocations, staged in LDS, stored as whole lines.
// lds layout: [column][block of 16 invocations][row of the pair][invocation % 16] = the 4 lines of a column in order.
__device__ __forceinline__ void trace_flush(uint32_t* lds, const uint32_t* r0, const uint32_t* r1, uint32_t* out, size_t Q,
                                            uint32_t c0, uint32_t j, size_t row_base, uint32_t n_blocks) {
    const uint32_t l = threadIdx.x, at = (l >> 4) * 32 + (l & 15u);
    __syncthreads();  // the previous flush's reads are done
#pragma unroll
    for (int c = 0; c < 16; c++) {
        lds[c * 128 + at] = r0[c];
        lds[c * 128 + at + 16] = r1[c];
    }
    __syncthreads();
    const uint4* l4 = reinterpret_cast<const uint4*>(lds);
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const uint32_t q = it * 64 + l, c = q >> 5, b = (q >> 3) & 3u, d = (q & 7u) * 4;  // 8 lanes per line
        if (b < n_blocks)
            *reinterpret_cast<uint4*>(out + (size_t)(c0 + c) * Q + row_base + b * 96 + j * 16 + d) = l4[q];
    }
}

// Grid: proof-major, ceil(n_pad / 64) waves of 64 invocations per proof.  Invocation k < copies * flow_count hashes flow
// record k % flow_count (every copy of the verifier invokes the same permutations); the padding invocations hash zeros
// with wires and swap address 0.  GROUPED (rsv_witness_trace_groups_dev): p is a group of `copies` proofs whose records lie
// one proof after the other, [n][copies][flow_count], and copy c hashes those of the group's proof c: record k of the group.
template <bool GROUPED, class A>
__device__ __forceinline__ void trace_poseidon(const A& a, uint32_t* lds) {
    const uint32_t per = (a.n_pad + TRACE_WAVE - 1) / TRACE_WAVE;
    const uint32_t p = blockIdx.x / per, k0 = (blockIdx.x % per) * TRACE_WAVE, k = k0 + threadIdx.x;
    const size_t Q = (size_t)1 << a.log_poseidon;
    uint32_t* out = a.poseidon + (size_t)p * POSEIDON_COLS_K * Q;
    const size_t row_base = (size_t)k0 * 6;
    const uint32_t n_blocks = min(4u, (a.n_pad - k0) / 16);  // n_pad is a multiple of 16
    if (!a.accept[p]) {  // a rejected proof: zero columns (uniform: one proof per workgroup)
        for (uint32_t q = threadIdx.x; q < POSEIDON_COLS_K * n_blocks * 24; q += TRACE_WAVE) {
            const uint32_t c = q / (n_blocks * 24), r = q % (n_blocks * 24);
            *reinterpret_cast<uint4*>(out + (size_t)c * Q + row_base + 4 * r) = make_uint4(0, 0, 0, 0);
        }
        return;
    }
    uint32_t in[16], sw = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) in[i] = 0;
    if (k < a.flow_count * a.copies) {
        const size_t rec = GROUPED ? (size_t)p * a.flow_count * a.copies + k : (size_t)p * a.flow_count + k % a.flow_count;
        const uint4* f = a.flow + rec * 8;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 v = f[q];
            in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
        }
        sw = a.swap[rec] != 0;
    }
    if constexpr (A::hashed)
        if (k >= a.flow_count * a.copies && k - a.flow_count * a.copies < a.stmt_flow) {
            const size_t rec = a.tail + (size_t)p * a.stmt_flow + (k - a.flow_count * a.copies);
            const uint4* f = a.flow + rec * 8;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 v = f[q];
                in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
            }
            sw = a.swap[rec] != 0;
        }
    // row 0: in = r1 || r2 as given, intermediate[0] = the swap bit, out = external matrix of the (swapped) input
    uint32_t s[16], mid0[16], mid1[16];
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = sw ? in[(i + 8) & 15] : in[i];
    trace_ext(s);
#pragma unroll
    for (int i = 0; i < 16; i++) mid0[i] = 0;
    mid0[0] = sw;
    // rows 0 and 1
    uint32_t s1[16];
#pragma unroll
    for (int i = 0; i < 16; i++) s1[i] = s[i];
    trace_full_pair(s1, mid1, 0);
    trace_flush(lds, in, s, out, Q, 0, 0, row_base, n_blocks);
    trace_flush(lds, mid0, mid1, out, Q, 16, 0, row_base, n_blocks);
    trace_flush(lds, s, s1, out, Q, 32, 0, row_base, n_blocks);
    // rows 2 and 3: the second full pair, then the 14 partial rounds
    uint32_t s2[16];
#pragma unroll
    for (int i = 0; i < 16; i++) s2[i] = s1[i];
    trace_full_pair(s2, mid0, 2);
#pragma unroll
    for (int i = 0; i < 16; i++) { s[i] = s2[i]; mid1[i] = 0; }
#pragma unroll
    for (int r = 0; r < 14; r++) {
        s[0] = pow5_ref(m_add(s[0], RC_PARTIAL[r]));
        mid1[r] = s[0];
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) t = m_add(t, s[i]);
        s[0] = m_add(t, m_add(m_dbl(s[0]), s[0]));  // diag 3
#pragma unroll
        for (int i = 1; i < 16; i++) s[i] = m_add(t, m_shl(s[i], i + 1));  // diag 2^(i+1)
    }
    trace_flush(lds, s1, s2, out, Q, 0, 2, row_base, n_blocks);
    trace_flush(lds, mid0, mid1, out, Q, 16, 2, row_base, n_blocks);
    trace_flush(lds, s2, s, out, Q, 32, 2, row_base, n_blocks);
    // rows 4 and 5: the last two full pairs
#pragma unroll
    for (int i = 0; i < 16; i++) s1[i] = s[i];
    trace_full_pair(s1, mid0, 4);
#pragma unroll
    for (int i = 0; i < 16; i++) s2[i] = s1[i];
    trace_full_pair(s2, mid1, 6);
    trace_flush(lds, s, s1, out, Q, 0, 4, row_base, n_blocks);
    trace_flush(lds, mid0, mid1, out, Q, 16, 4, row_base, n_blocks);
    trace_flush(lds, s1, s2, out, Q, 32, 4, row_base, n_blocks);
}
template <bool GROUPED, class A>
__global__ __launch_bounds__(64) void k_trace_poseidon(A a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[TRACE_STAGE];
    trace_poseidon<GROUPED>(a, lds);
}

// The rows behind the padded flow, [6 * n_pad, 2^lq) of all 48 columns of every proof: zero.  The start is a multiple of
// 96 rows and both ends are multiples of 32 rows (2^lq >= 192), so every store is a whole 16-byte quad.
__global__ __launch_bounds__(256) void k_trace_zero_tail(uint32_t* __restrict__ poseidon, uint32_t log_poseidon, uint32_t first_row,
                                                         uint64_t n_cols) {
    const size_t Q = (size_t)1 << log_poseidon, quads = (Q - first_row) / 4;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= quads * n_cols) return;
    const uint64_t col = t / quads, q = t % quads;
    *reinterpret_cast<uint4*>(poseidon + col * Q + first_row + 4 * q) = make_uint4(0, 0, 0, 0);
}

}  // namespace rsv
