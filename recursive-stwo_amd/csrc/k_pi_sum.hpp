// k_pi_sum.hpp — the statement's share of the logup balance, sum_i 1 / (v_i + (idx_i mod P) alpha - z), for a batch in
// which every proof has its own public inputs (rsv_verify_batch_inputs_dev).  Part of the pipeline described in verify.hpp.
//
// The shared form (one table for the whole batch) keeps the sum inside k_oods / k_oods_row: one lane, or the sixteen lanes
// of a row, take one dependent QM31 inversion per input, and the table stays in cache.  With per-proof inputs the table
// is n x n_pi records of 20 bytes, so the sum gets a kernel of its own, behind the transcript (which draws z and alpha)
// and ahead of the OODS kernel (which reads the per-proof sum and has no loop):
//   - one wave per proof, PI_WAVES proofs per workgroup;
//   - input k of the proof belongs to lane k mod 64: a round of the wave covers 64 consecutive records, 320 consecutive
//     words, which the wave reads as five coalesced 256-byte loads into LDS (a record is 20 bytes: neither it nor a
//     proof's first record is 16-byte aligned in general, words always are) and each lane then takes its five words from
//     there (stride 5: no bank conflict);
//   - a lane inverts its denominators PI_CHUNK at a time with Montgomery's trick: one q_inv per lane per chunk;
//   - the lanes' sums are added across the wave, lane 0 writes the proof's four words.
// Two rules ("Per-proof public inputs"):
//   - a ZERO denominator.  The per-term loop adds q_inv(0), and q_inv(0) is 0 (field.hpp: m_inv(0) = 0^(P-2) = 0, and the
//     norms of CM31 and QM31 vanish only at 0), so a zero term adds nothing.  In a batched inversion a zero would
//     make the whole chunk's product zero: it is left out of the running product (the factor is 1 in its place) and adds nothing;
//   - a value word >= P.  The shared form refuses it on the host (RSV_E_RANGE); inputs in HBM are data: the word counts as
//     0 and the proof gets R_PARSE ("a non-canonical field element"), as a non-canonical word of the proof itself does.
//     idx is taken mod P, as in the shared form.
// Every other term is the field inverse, which is unique: the sum is, word for word, the one the per-term loop gives.
#pragma once
#include "verify_common.hpp"

namespace rsv {

constexpr int PI_WAVES = 4;   // proofs per workgroup
constexpr int PI_CHUNK = 8;   // denominators per lane per inversion (4 096 inputs: 64 per lane, eight chunks)
constexpr int PI_WORDS = 5;   // words of a record: idx, value[4]
static_assert(sizeof(PubInput) == 4 * PI_WORDS, "a packed record of five words");

__device__ __forceinline__ uint32_t pi_canon(uint32_t w, bool& bad) {
    if (w >= P) { bad = true; return 0u; }
    return w;
}
__device__ __forceinline__ QM31 q_sum_wave(QM31 x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        x = q_add(x, q_mk(__shfl_xor(x.a.a, s), __shfl_xor(x.a.b, s), __shfl_xor(x.b.a, s), __shfl_xor(x.b.b, s)));
    return x;
}

// PIPE: in the verify pipeline — (z, alpha) from ProofCtx, a proof the parser rejected is not touched, a non-canonical
// word raises R_PARSE in ProofCtx::flags; else the kernel alone (rsv_public_input_sum_dev) — (z, alpha) from z_alpha [n][8],
// a non-canonical word of either sets bad[p] (bad may be null).  sum [n][4].
template <bool PIPE>
__global__ __launch_bounds__(64 * PI_WAVES) void k_pi_sum(const uint32_t* __restrict__ rec, uint32_t n, uint32_t n_pi,
                                                          const ProofMeta* __restrict__ metas, ProofCtx* __restrict__ ctxs,
                                                          const uint32_t* __restrict__ z_alpha, uint32_t* __restrict__ sum,
                                                          uint8_t* __restrict__ bad) {
    __shared__ uint32_t stage[PI_WAVES][64 * PI_WORDS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t p = blockIdx.x * PI_WAVES + wave;
    // wave-uniform; a wave without a proof still walks the rounds (the barriers are the workgroup's) and touches no memory
    const bool live = p < n && (!PIPE || metas[p].reason == R_OK);
    bool over = false;
    QM31 z = q_zero(), alpha = q_zero();
    if (live) {
        const uint32_t* za = PIPE ? ctxs[p].z : z_alpha + (size_t)p * 8;
        const uint32_t* al = PIPE ? ctxs[p].alpha : za + 4;
        if (PIPE) { z = ldq(za); alpha = ldq(al); }  // the transcript's own draws: canonical
        else {
            z = q_mk(pi_canon(za[0], over), pi_canon(za[1], over), pi_canon(za[2], over), pi_canon(za[3], over));
            alpha = q_mk(pi_canon(al[0], over), pi_canon(al[1], over), pi_canon(al[2], over), pi_canon(al[3], over));
        }
    }
    const uint32_t* mine = rec + (size_t)p * n_pi * PI_WORDS;  // (dereferenced by a live wave only)
    const uint32_t rounds = (n_pi + 63u) / 64u;
    QM31 total = q_zero();
#pragma unroll 1
    for (uint32_t r0 = 0; r0 < rounds; r0 += PI_CHUNK) {
        QM31 den[PI_CHUNK], before[PI_CHUNK];  // before[j]: the product of the chunk's non-zero denominators ahead of j
        QM31 run = q_one();
        uint32_t has = 0;  // bit j: term j exists and its denominator is not zero
#pragma unroll
        for (int j = 0; j < PI_CHUNK; j++) {
            const uint32_t first = (r0 + j) * 64u;  // the round's first record
            den[j] = q_one();
            before[j] = run;
            if (first < n_pi) {  // (uniform over the workgroup)
                const uint32_t cnt = umin(64u, n_pi - first);
                if (live) {
#pragma unroll
                    for (int t = 0; t < PI_WORDS; t++) {
                        const uint32_t w = lane + 64u * t;
                        if (w < cnt * PI_WORDS) stage[wave][w] = mine[(size_t)first * PI_WORDS + w];
                    }
                }
                __syncthreads();
                if (live && lane < cnt) {
                    const uint32_t* s = stage[wave] + lane * PI_WORDS;
                    const QM31 v = q_mk(pi_canon(s[1], over), pi_canon(s[2], over), pi_canon(s[3], over), pi_canon(s[4], over));
                    const QM31 dnm = q_sub(q_add(v, q_mul_m(alpha, s[0] % P)), z);
                    if (!q_eq(dnm, q_zero())) {
                        den[j] = dnm;
                        has |= 1u << j;
                    }
                }
                __syncthreads();  // the next round overwrites the stage
                run = q_mul(run, den[j]);
            }
        }
        QM31 inv = q_inv(run);  // (a lane without a term inverts 1)
#pragma unroll
        for (int j = PI_CHUNK - 1; j >= 0; j--) {
            if ((has >> j) & 1u) total = q_add(total, q_mul(inv, before[j]));
            inv = q_mul(inv, den[j]);
        }
    }
    total = q_sum_wave(total);
    const bool any_over = __any(over);
    if (live && lane == 0) {
        stq(sum + (size_t)p * 4, total);
        if (PIPE) {
            if (any_over) atomicOr(&ctxs[p].flags, 1u << R_PARSE);
        } else if (bad) bad[p] = any_over ? 1 : 0;
    }
}

// rsv_circuit_inputs_dev: the statement of each witness, (k, variables[k]) for k = 1 .. num_input, as packed records
// [n][num_input][5]; variables in either witness layout.  One lane per word.
__global__ __launch_bounds__(256) void k_circuit_inputs(const uint32_t* __restrict__ vars, uint32_t n, uint32_t n_vars, uint32_t num_input,
                                                        bool by_variable, uint32_t* __restrict__ rec) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * num_input * PI_WORDS) return;
    const uint32_t w = (uint32_t)(i % PI_WORDS);
    const size_t kp = i / PI_WORDS;
    const uint32_t k = 1u + (uint32_t)(kp % num_input), p = (uint32_t)(kp / num_input);
    rec[i] = w == 0 ? k : vars[(by_variable ? (size_t)k * n + p : (size_t)p * n_vars + k) * 4 + (w - 1)];
}

}  // namespace rsv
