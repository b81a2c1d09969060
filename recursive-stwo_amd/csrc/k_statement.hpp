// k_statement.hpp — the digest of the statements a group of the recursion circuit verifies (rsv_statement_digest_dev).
//
// Group g verifies `copies` proofs with n_own records each; v[c * n_own + k] = word 0 of the value of record k of the proof
// of copy c, T = copies * n_own words in copy-major order, which is the order the records lie in memory.  The digest is
//     Poseidon31MerkleHasherVar::hash_m31_columns_get_rate(v[0 .. T))          (primitives/merkle/src/lib.rs:50-91)
// — the leaf hash of a childless node with T columns, merkle.hpp's hash_node(NULL, NULL, v, T): ceil(T / 8) chunks absorbed
// into the capacity, then the rate permutation; S = ceil(T / 8) + 1 permutations, one after the other.  The records' idx is
// not hashed (it is a constant of the program that reads the statement).
//
// Two forms, as the Merkle kernels have (FORM: poseidon2.hpp):
//   - lane form (FORM 0): one lane per group, a workgroup of one wave = 64 groups.  For large batches, where the
//     permutations of different groups fill the lanes; the unpaced instance, since a launch of 65 536 groups puts one
//     wave on a SIMD (as the lane-form transcript);
//   - row form (FORM_ROW): the 16 lanes of a DPP row per group, a workgroup of 256 threads = 16 groups.  For small batches,
//     where the S dependent permutations of one group are the whole latency.
// A group's records are 20-byte structs, T of them apart from the next group's: the workgroup stages them through LDS in
// tiles of STMT_TILE records per group.  Consecutive threads take consecutive records of a group's run (a wave's four value
// loads cover the same 1 280 contiguous bytes: every line fetched is used whole; with T <= STMT_TILE the runs of the
// workgroup's groups are one contiguous span), keep the value word and check the others; a group's lane, or row, then reads
// its own STMT_TILE words from LDS, rows padded by one word (a ds_read_b32 has 32 banks: lane l reads bank (l + i) mod 32).
// LDS: 64 x 33 words = 8.25 KB (lane form), 16 x 33 words = 2.1 KB (row form): no bound on occupancy beside the
// permutation's registers.
// Two rules, k_pi_sum's ("Statement digests"): a value word >= P counts as 0, and it, or a non-zero word 1..3
// (the circuit holds the statement in M31 variables), sets bad[g].
#pragma once
#include "merkle.hpp"
#include "verify_common.hpp"

namespace rsv {

constexpr uint32_t STMT_TILE = 32;  // records of a group per stage: four chunks of the sponge
constexpr uint32_t STMT_ROW = STMT_TILE + 1;
static_assert(STMT_TILE % 8 == 0, "a tile ends on a chunk boundary: only the last chunk of a group is padded");

// rec [n_groups][T] records; stmt [n_groups][8] records (idx = 4 + k, value = (digest[k], 0, 0, 0)): the statement of the
// outer proof as the verifier, and the next level's d_pi, take it; bad [n_groups] (may be null).  T >= 1.
// FLOW (the evaluation of a hashed witness program): the S = ceil(T / 8) + 1 invocations of group g are records
// flow[g][0 .. S) with swap bytes 0 — the tail of the caller's flow buffers, which the verifying pass does not write.
template <int FORM, bool FLOW>
__global__ __launch_bounds__(FORM == FORM_ROW ? 256 : 64) void k_statement_digest(const uint32_t* __restrict__ rec, uint32_t n_groups, uint32_t T,
                                                                                  uint32_t* __restrict__ stmt, uint8_t* __restrict__ bad,
                                                                                  uint4* __restrict__ flow, uint8_t* __restrict__ flow_swap) {
    constexpr uint32_t BLOCK = FORM == FORM_ROW ? 256 : 64;
    constexpr uint32_t VB = FORM == FORM_ROW ? BLOCK / 16 : BLOCK;  // groups per workgroup
    __shared__ uint32_t s_val[VB * STMT_ROW];
    __shared__ uint32_t s_bad[VB];
    row_rc_init<FORM>();
    const uint32_t vl = vlane<FORM>(), g0 = blockIdx.x * VB, g = g0 + vl;
    const bool live = g < n_groups;  // (uniform over a row)
    if (threadIdx.x < VB) s_bad[threadIdx.x] = 0;
    Hash8 d = zero8();
    const uint32_t n_rec = (T + 7) / 8 + 1;
    const FlowSink sink{FLOW && live ? flow + (size_t)g * n_rec * 8 : nullptr, FLOW && live ? flow_swap + (size_t)g * n_rec : nullptr};
    uint32_t idx = 0;
#pragma unroll 1
    for (uint32_t t0 = 0; t0 < T; t0 += STMT_TILE) {  // (uniform over the workgroup)
        const uint32_t cnt = umin(STMT_TILE, T - t0);
        const uint32_t magic = ((1u << 20) + cnt - 1) / cnt;  // q / cnt = (q * magic) >> 20 for q < VB * cnt <= 2^11 (error q (magic cnt - 2^20) < 2^16)
        __syncthreads();  // the tile before is absorbed (first round: s_bad is cleared)
        for (uint32_t q = threadIdx.x; q < VB * cnt; q += BLOCK) {
            const uint32_t gl = (q * magic) >> 20, r = q - gl * cnt;
            if (g0 + gl < n_groups) {
                const uint32_t* w = rec + ((size_t)(g0 + gl) * T + t0 + r) * 5;
                uint32_t v = w[1];
                const bool wrong = v >= P || (w[2] | w[3] | w[4]) != 0;
                if (v >= P) v = 0;
                s_val[gl * STMT_ROW + r] = v;
                if (wrong) s_bad[gl] = 1;  // (every writer stores the same word)
            }
        }
        __syncthreads();
        if (live) {  // the tile's chunks, continuing from the capacity so far (whole chunks but for the group's last)
            if constexpr (FLOW) {
                d = flow_sponge_capacity<FORM>(sink, idx, s_val + vl * STMT_ROW, cnt, d);
                idx += (cnt + 7) / 8;
            } else d = sponge_capacity<FORM>(s_val + vl * STMT_ROW, cnt, d);
        }
    }
    if (!live) return;
    Hash8 h;
    if constexpr (FLOW) h = rate_of(flow_perm<FORM>(sink, idx, zero8(), d, false));
    else h = leaf_from_capacity<FORM>(d);
    if (FORM == FORM_ROW && (threadIdx.x & 15u) != 0) return;  // the row's lanes hold the same digest: one of them writes
    uint32_t* out = stmt + (size_t)g * 40;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        out[5 * k] = 4u + k;
        out[5 * k + 1] = h.w[k];
        out[5 * k + 2] = 0; out[5 * k + 3] = 0; out[5 * k + 4] = 0;
    }
    if (bad) bad[g] = (uint8_t)s_bad[vl];
}

}  // namespace rsv
