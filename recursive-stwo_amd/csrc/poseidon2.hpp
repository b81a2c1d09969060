// poseidon2.hpp — Poseidon2 over M31, width 16, x^5, 4 + 14 + 4 rounds.
//
// Values side of poseidon2_permute (primitives/poseidon31/src/implementation.rs:108-149)
// with the external matrix circ(2*M4, M4, M4, M4) (:7-58) and the internal
// matrix diag(3,4,8,...,65536) + J (:128-138).  The 142 round constants are the
// Poseidon2 parameters for p = 2^31-1, t = 16 published in
// primitives/poseidon31/src/parameters.rs:6-190.
//
// MI355X mapping: ONE LANE PER PERMUTATION.  The 16-word state lives in 16
// VGPRs of one lane, so a wave64 advances 64 independent permutations with no
// cross-lane traffic.  The fast path (poseidon2_inline, below) is straight-line
// code: round constants are 32-bit literals of a fused add + reduce, the
// linear layers accumulate unreduced in 64 bits, the partial-round diagonal is
// a multiply-accumulate by a power of two.  One out-of-line instance
// (poseidon2(), ~30 KB of code in 38 VGPRs) is shared by every call site.
#pragma once
#include "field.hpp"

namespace rsv {

struct State16 {
    uint32_t s[16];
};

#define RSV_RC_FULL_INIT { \
    {0x768bab52, 0x70e0ab7d, 0x3d266c8a, 0x6da42045, 0x600fef22, 0x41dace6b, 0x64f9bdd4, 0x5d42d4fe, \
     0x76b1516d, 0x6fc9a717, 0x70ac4fb6, 0x00194ef6, 0x22b644e2, 0x1f7916d5, 0x47581be2, 0x2710a123}, \
    {0x6284e867, 0x018d3afe, 0x5df99ef3, 0x4c1e467b, 0x566f6abc, 0x2994e427, 0x538a6d42, 0x5d7bf2cf, \
     0x7fda2dab, 0x0fd854c4, 0x46922fca, 0x3d7763a1, 0x19fd05ca, 0x0a4bbb43, 0x15075851, 0x3d903d76}, \
    {0x2d290ff7, 0x40809fa0, 0x59dac6ec, 0x127927a2, 0x6bbf0ea0, 0x0294140f, 0x24742976, 0x6e84c081, \
     0x22484f4a, 0x354cae59, 0x0453ffe1, 0x3f47a3cc, 0x0088204e, 0x6066e109, 0x3b7c4b80, 0x6b55665d}, \
    {0x3bc4b897, 0x735bf378, 0x508daf42, 0x1884fc2b, 0x7214f24c, 0x7498be0a, 0x1a60e640, 0x3303f928, \
     0x29b46376, 0x5c96bb68, 0x65d097a5, 0x1d358e9f, 0x4a9a9017, 0x4724cf76, 0x347af70f, 0x1e77e59a}, \
    {0x57090613, 0x1fa42108, 0x17bbef50, 0x1ff7e11c, 0x047b24ca, 0x4e140275, 0x4fa086f5, 0x079b309c, \
     0x1159bd47, 0x6d37e4e5, 0x075d8dce, 0x12121ca0, 0x7f6a7c40, 0x68e182ba, 0x5493201b, 0x0444a80e}, \
    {0x0064f4c6, 0x6467abe6, 0x66975762, 0x2af68f9b, 0x345b33be, 0x1b70d47f, 0x053db717, 0x381189cb, \
     0x43b915f8, 0x20df3694, 0x0f459d26, 0x77a0e97b, 0x2f73e739, 0x1876c2f9, 0x65a0e29a, 0x4cabefbe}, \
    {0x5abd1268, 0x4d34a760, 0x12771799, 0x69a0c9ac, 0x39091e55, 0x7f611cd0, 0x3af055da, 0x7ac0bbdf, \
     0x6e0f3a24, 0x41e3b6f7, 0x49b3756d, 0x568bc538, 0x20c079d8, 0x1701c72c, 0x7670dc6c, 0x5a439035}, \
    {0x7c93e00e, 0x561fbb4d, 0x1178907b, 0x02737406, 0x32fb24f1, 0x6323b60a, 0x6ab12418, 0x42c99cea, \
     0x155a0b97, 0x53d1c6aa, 0x2bd20347, 0x279b3d73, 0x4f5f3c70, 0x0245af6c, 0x238359d3, 0x49966a59}}
__constant__ __attribute__((aligned(64))) uint32_t RC_FULL[8][16] = RSV_RC_FULL_INIT;
constexpr uint32_t RC_FULL_K[8][16] = RSV_RC_FULL_INIT;  // the same values as compile-time constants (literal operands)

// 14 constants + 2 words of padding (block loads)
#define RSV_RC_PARTIAL_INIT { \
   0x7f7ec4bf, 0x0421926f, 0x5198e669, 0x34db3148, 0x4368bafd, \
                                        0x66685c7f, 0x78d3249a, 0x60187881, 0x76dad67a, 0x0690b437, \
                                        0x1ea95311, 0x40e5369a, 0x38f103fc, 0x1d226a21, 0, 0}
__constant__ __attribute__((aligned(64))) uint32_t RC_PARTIAL[16] = RSV_RC_PARTIAL_INIT;
constexpr uint32_t RC_PARTIAL_K[16] = RSV_RC_PARTIAL_INIT;

// ---- canonical S-box and external matrix, one reduction per operation: what the trace and emulated-field kernels use
// (k_trace.hpp, k_emulated.hpp).  tools/perm_lab.hip builds the whole permutation from them as its baseline.
__device__ __forceinline__ uint32_t pow5_ref(uint32_t x) {
    uint32_t x2 = m_sqr(x);
    return m_mul(m_sqr(x2), x);
}

// M4 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]] (Poseidon2 paper, 5.1) in 8 additions, 2 doublings, 2 x4.
__device__ __forceinline__ void mds4_ref(uint32_t& x0, uint32_t& x1, uint32_t& x2, uint32_t& x3) {
    uint32_t t0 = m_add(x0, x1), t1 = m_add(x2, x3);
    uint32_t t2 = m_add(m_dbl(x1), t1), t3 = m_add(m_dbl(x3), t0);
    uint32_t t4 = m_add(m_shl(t1, 2), t3), t5 = m_add(m_shl(t0, 2), t2);
    x0 = m_add(t3, t5);
    x1 = t5;
    x2 = m_add(t2, t4);
    x3 = t4;
}

__device__ __forceinline__ void mds16_ref(uint32_t* s) {
#pragma unroll
    for (int g = 0; g < 4; g++) mds4_ref(s[4 * g], s[4 * g + 1], s[4 * g + 2], s[4 * g + 3]);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t sum = m_add(m_add(s[j], s[j + 4]), m_add(s[j + 8], s[j + 12]));
#pragma unroll
        for (int g = 0; g < 4; g++) s[4 * g + j] = m_add(s[4 * g + j], sum);
    }
}

// ===========================================================================================
// Fast path.  Instruction costs measured on MI355X (tools/valu_lab.hip, 4 waves/SIMD):
//   ~2.5 cycles : v_add_u32 v_sub_u32 v_and_b32 v_or_b32 v_lshrrev_b32 v_ashrrev_i32 v_mov_b32 (also with a literal)
//   ~4.3-4.6    : v_min_u32 v_lshlrev_b32 v_alignbit_b32 v_and_or_b32 v_mul_lo/hi_u32 v_lshl_add_u64 v_add3_u32 v_xad_u32
//                 v_mad_u64_u32 (4.55; 5.05 with a live 64-bit addend)   -- the 32x32->64 multiply is
//                 NOT quarter rate on gfx950, so the cost of a modular multiply is its reduction.
//                 v_mad_i64_i32 with an SGPR-pair addend 4.51, 4.30 as a square (the S-box's products); without an
//                 addend 4.34; v_mad_u64_u32 with an SGPR-pair addend 4.48
// Consequences used below:
//   * linear layers accumulate UNREDUCED in 64 bits (one v_lshl_add_u64 / v_mad_u64_u32 per term,
//     shifts by 1..4 and small multipliers are free), and are folded once per round;
//   * accumulators hold 2*v, so the Mersenne fold (v >> 31) + (v & P) is hi32 + (lo32 >> 1): two
//     fast-class instructions instead of v_and + v_alignbit + v_add;
//   * a product x*y is formed as (2x)*y for the same reason;
//   * a conditional subtract is a slow-class v_min, so the S-box has none: its values are signed words, kept in range by
//     addends that are multiples of P (pow5c), and its input is reduced by a sign-mask select (centre_rc);
//   * values between steps are only "weakly" reduced; the ranges are tracked in the comments:
//       C  = [0, P]           (canonical, or P itself which is congruent to 0)
//       L2 = [0, 2P]          (one conditional subtract away from C)
//     tests/perm_model.py restates this arithmetic on machine words: the tests built on it prove every range and compare
//     the model with the reference permutation.  The kernels are compared with that reference on the GPU
//     (tests/test_perm_signmask_gpu.py); tools/perm_lab.hip compares them with a canonical restatement.
// ===========================================================================================
// Issue pacing.  Measured on MI355X (whole pipeline, 65 536 proofs): when a wave presents an instruction that depends
// on its own previous VALU result, the SIMD stalls on it instead of issuing another wave's instruction.  A wait state
// behind such an instruction takes the wave out of arbitration for those cycles.  Measured when every reduction still
// ended in a v_min: one extra wait state behind every v_mad_u64_u32 (the compiler adds one of its own behind an asm
// statement whose result is read next) and two behind the v_min gave
//     no pacing 37.75 ms | mad 36.40 | mad + v_min 35.80 | also behind fold2 / the doublings: 35.75-35.85 (plateau)
//     two wait states behind the multiplies: 36.17 (worse) | s_nop 3: 40.2
// The wait states cost nothing at >= 4 waves per SIMD (other waves fill them); at one wave per SIMD (the lane-form
// transcript of batches > 24 576) they lengthen the chain by ~25 % — that kernel runs underneath k_row_hash.
// PACE: one wait state behind every 64-bit multiply and one behind the fold that ends pow5c's x^4 (the end of the S-box's
// only multi-instruction reduction).  They pay where several waves share a SIMD and cost ~25 % where a wave is (nearly)
// alone on it, so the verify kernels pick the instance by the size of the launch (poseidon2_half below): paced for
// launches that fill the machine, unpaced for a small batch's trees and for the one-wave-per-SIMD lane-form transcript.
template <bool PACE>
struct PermT {
    static __device__ __forceinline__ uint64_t add64(uint64_t a, uint64_t b) {
        uint64_t d;
        asm("v_lshl_add_u64 %0, %1, 0, %2" : "=v"(d) : "v"(a), "v"(b));
        return d;
    }
    template <int SH>
    static __device__ __forceinline__ uint64_t shl_add64(uint64_t a, uint64_t b) {  // (a << SH) + b, SH in 1..4
        uint64_t d;
        asm("v_lshl_add_u64 %0, %1, %3, %2" : "=v"(d) : "v"(a), "v"(b), "n"(SH));
        return d;
    }
    // 32x32 -> 64 products and multiply-accumulates (v_mad_u64_u32).  The small constant multipliers are
    // passed as OPAQUE wave-uniform values (see opaque()): with a visible constant hipcc strength-reduces
    // a*2+c into slow-class shifts plus zero-extension moves instead of one v_mad_u64_u32.
    static __device__ __forceinline__ uint32_t opaque(uint32_t k) {
        uint32_t r;
        asm volatile("s_mov_b32 %0, %1" : "=s"(r) : "n"(k));
        return r;
    }
    // the same for a 64-bit constant, in an SGPR pair (the S-box's addends: see pow5c)
    static __device__ __forceinline__ uint64_t opaque64(uint64_t k) {
        return (uint64_t)opaque((uint32_t)(k >> 32)) << 32 | opaque((uint32_t)k);
    }
    // The asm form (instead of `(uint64_t)a * b + c`) also keeps hipcc from re-associating
    // x0*k + x1*k into (x0 + x1)*k, which costs a 64-bit add, a 64x32 multiply and zero-extension moves.
    static __device__ __forceinline__ uint64_t mul64(uint32_t a, uint32_t b_uniform) {  // a * b, b in an SGPR
        uint64_t d, carry;
        if constexpr (PACE) asm("v_mad_u64_u32 %0, %1, %2, %3, 0\n\ts_nop 0" : "=v"(d), "=s"(carry) : "v"(a), "s"(b_uniform));
        else asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(d), "=s"(carry) : "v"(a), "s"(b_uniform));
        return d;
    }
    static __device__ __forceinline__ uint64_t mad64(uint32_t a, uint32_t b_uniform, uint64_t c) {  // a * b + c, b in an SGPR
        uint64_t d, carry;
        if constexpr (PACE) asm("v_mad_u64_u32 %0, %1, %2, %3, %4\n\ts_nop 0" : "=v"(d), "=s"(carry) : "v"(a), "s"(b_uniform), "v"(c));
        else asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(d), "=s"(carry) : "v"(a), "s"(b_uniform), "v"(c));
        return d;
    }
    // signed a * b + c (v_mad_i64_i32), c a signed 64-bit constant in an SGPR pair; the square a * a + c reads one register
    static __device__ __forceinline__ uint64_t mad64s(int32_t a, int32_t b, uint64_t c_uniform) {
        uint64_t d, carry;
        if constexpr (PACE) asm("v_mad_i64_i32 %0, %1, %2, %3, %4\n\ts_nop 0" : "=v"(d), "=s"(carry) : "v"(a), "v"(b), "s"(c_uniform));
        else asm("v_mad_i64_i32 %0, %1, %2, %3, %4" : "=v"(d), "=s"(carry) : "v"(a), "v"(b), "s"(c_uniform));
        return d;
    }
    static __device__ __forceinline__ uint64_t sqr64s(int32_t a, uint64_t c_uniform) {
        uint64_t d, carry;
        if constexpr (PACE) asm("v_mad_i64_i32 %0, %1, %2, %2, %3\n\ts_nop 0" : "=v"(d), "=s"(carry) : "v"(a), "s"(c_uniform));
        else asm("v_mad_i64_i32 %0, %1, %2, %2, %3" : "=v"(d), "=s"(carry) : "v"(a), "s"(c_uniform));
        return d;
    }
    static __device__ __forceinline__ uint32_t dbl32(uint32_t x) {  // x + x as a fast-class add (not a shift)
        uint32_t d;
        asm("v_add_u32 %0, %1, %1" : "=v"(d) : "v"(x));
        return d;
    }
    // V = 2v with v < 2^62  ->  (v >> 31) + (v & P)
    static __device__ __forceinline__ uint32_t fold2(uint64_t V) {
        uint32_t r = (uint32_t)(V >> 32) + ((uint32_t)V >> 1);
        return r;
    }

    // ---- The S-box.  Its input is the CENTRED representative x of t + rc, in [-2^30, 2^30 - 2] (centre_rc below), and
    // every intermediate is a signed word.  The three products are v_mad_i64_i32 with a signed 64-bit addend that is a
    // multiple of P, held in an SGPR pair (opaque64()): KP = -P * 2^32, KN = -P * 2^31, KQ = P * 2^31.
    static constexpr uint64_t KP = 0 - ((uint64_t)P << 32);
    static constexpr uint64_t KN = 0 - ((uint64_t)P << 31), KQ = (uint64_t)P << 31;
    struct SboxK {
        uint64_t kp, kn, kq;
    };
    static __device__ __forceinline__ SboxK sbox_k() { return {opaque64(KP), opaque64(KN), opaque64(KQ)}; }
    // centre_rc reduces with the round constant moved by CENTRE: (t + rc + 2^30) mod P, less 2^30, is the centred x
    static constexpr uint32_t CENTRE = 1u << 30;
    static constexpr uint32_t centred(uint32_t rc) { return (uint32_t)(((uint64_t)rc + CENTRE) % P); }

    // x centred  ->  x^5 in L2:
    //     x                              [-2^30, 2^30 - 2]
    //     xx = 2x                        [-2^31, 2^31 - 4]: even, and an int32 because x is centred
    //     s1 = fold2(xx * x + KP)        2x^2 <= 2^61: fold2(2x^2) - P in [-P, 2^29], congruent to x^2
    //     V2 = s1 * s1 + KN              [-P * 2^31, -P]
    //     c4 = (V2 >> 31) + (V2 & P)     fold(s1^2) - P in [-P, P - 2], congruent to x^4, with no conditional subtract
    //     y  = fold2(xx * c4 + KQ)       xx * c4 in [-2^31 P, 2^31 P], so V3 in [0, 2^32 P] and even: y in [0, 2P - 1]
    // The last product is the one a signed S-box has to resolve: x * c4 over two full-width operands spans 2 P^2, one bit
    // more than a 32-bit fold takes.  Centring x lets it be doubled inside an int32, so the product is even, spans 2^32 P <
    // 2^63 and ends in the two-instruction fold2.  11 instructions: a doubling, three multiplies, two fold2 and the
    // three-instruction fold of V2 (alignbit, and, add).  tests/test_sbox_centred.py proves the ranges.
    static __device__ __forceinline__ uint32_t pow5c(int32_t x, const SboxK& k) {
        const int32_t xx = (int32_t)dbl32((uint32_t)x);
        const int32_t s1 = (int32_t)fold2(mad64s(xx, x, k.kp));
        const uint64_t V2 = sqr64s(s1, k.kn);
        uint32_t c4 = __builtin_amdgcn_alignbit((uint32_t)(V2 >> 32), (uint32_t)V2, 31) + ((uint32_t)V2 & P);
        if constexpr (PACE) asm volatile("s_nop 0" : "+v"(c4));  // the reduction's end
        return fold2(mad64s(xx, (int32_t)c4, k.kq));
    }

    // ---- The external linear layer, V[i] = 2 * (circ(2M4, M4, M4, M4) * s)[i], inputs any u32 (< 2^32).  With the column
    // sums X_j = s_j + s_{4+j} + s_{8+j} + s_{12+j}, group g of the product is M4 s_g + M4 X = M4 (s_g + X): the sums are
    // formed FIRST and one M4 per group does the rest, on 64-bit inputs with shifts and adds alone (16 + 16 multiplies and
    // 4 x 8 v_lshl_add_u64 for the layer; M4 per group first and the sums of its outputs afterwards is 24 + 44).  Everything
    // is doubled from the first multiply on, and exact in 64 bits:
    //     X2_j = 2 X_j                  < 4 * 2^33 = 2^35
    //     z_j  = 2 s_{4g+j} + X2_j      < 10 * 2^32 < 2^36
    //     t0, t1 < 2^37;  t2, t3 < 40 * 2^32;  t4, t5 < 120 * 2^32;  y_j < 160 * 2^32 < 2^40
    // The matrix rows sum to at most 16 * 5 = 80, which is the bound on y: V[i] < 160 * 2^32 (HI_FULL below).  V never carries
    // a round constant (they are literals of the fused reductions).  tests/test_mds_colsum.py proves the bounds and V equal
    // to the sum-after-M4 form on machine words.
    static __device__ __forceinline__ void colsums_2x(uint32_t k2, const uint32_t* s, uint64_t* X2) {
    #pragma unroll
        for (int j = 0; j < 4; j++) X2[j] = mul64(s[j], k2);
    #pragma unroll
        for (int g = 1; g < 4; g++) {
    #pragma unroll
            for (int j = 0; j < 4; j++) X2[j] = mad64(s[4 * g + j], k2, X2[j]);
        }
    }
    // Y = M4 * (z0..z3) for 64-bit inputs, eight v_lshl_add_u64 (the additions, doublings and x4 of mds4_ref).
    static __device__ __forceinline__ void mds4(uint64_t z0, uint64_t z1, uint64_t z2, uint64_t z3,
                                                uint64_t& y0, uint64_t& y1, uint64_t& y2, uint64_t& y3) {
        uint64_t t0 = add64(z0, z1), t1 = add64(z2, z3);
        uint64_t t2 = shl_add64<1>(z1, t1), t3 = shl_add64<1>(z3, t0);
        uint64_t t4 = shl_add64<2>(t1, t3), t5 = shl_add64<2>(t0, t2);
        y0 = add64(t3, t5);
        y1 = t5;
        y2 = add64(t2, t4);
        y3 = t4;
    }
    // one group of the layer: V[0..3] = M4 (2 x + X2) for the group's four words x.  The callers take the layer a group at a
    // time (mds_sbox, mds_fold, poseidon2_inline_half), so the sixteen accumulators never exist at once.
    static __device__ __forceinline__ void mds_group_2x(uint32_t k2, const uint64_t* X2, const uint32_t* x, uint64_t* V) {
        mds4(mad64(x[0], k2, X2[0]), mad64(x[1], k2, X2[1]), mad64(x[2], k2, X2[2]), mad64(x[3], k2, X2[3]), V[0], V[1], V[2], V[3]);
    }
    // Round constant + reduction to the centred representative in one step: the S-box's entry.  t = fold2(V) with V the
    // doubled accumulator of a linear layer WITHOUT its round constant: t <= P + HI where HI bounds the accumulator's high
    // word at the call site.  RC is the round constant moved by 2^30 (centred()), c = P - RC a compile-time literal, and
    // a = t - c read as an int32 lies in [-c, P + HI - c]: it does not wrap (c > HI, asserted; the upper end is HI + RC < P).
    // t + RC mod P is a two-way select on the sign of a, and x is that less 2^30:
    //     a >= 0 :  t + RC - P in [0, P - 1]      x = a - 2^30       = a + 0xC0000000
    //     a <  0 :  t + RC     in [0, P - 1]      x = a + P - 2^30   = a + 0x3FFFFFFF
    // The two addends are bit-complements, so the sign mask picks one: x = a + ((a >> 31) ^ 0xC0000000), arithmetic shift.
    // Written in C++ on purpose: hipcc folds the literal add into the fold2 that feeds it (v_add3_u32, the literal in an SGPR)
    // and the xor into the last add (v_xad_u32; 0xC0000000 is the inline constant -2.0), so fold2 and the entry together
    // are v_lshrrev_b32, v_add3_u32, v_ashrrev_i32, v_xad_u32 — against v_mad_u64_u32 (2 * rc folded into V, 5.1) and a
    // conditional subtract for a round constant carried by the accumulator.  No wait state of its own.
    // tests/test_sbox_signmask.py proves x equal to min(t - c, t - c + P) - 2^30, the same select by v_min, at every call
    // site; tools/perm_ceiling.py prints the static opcode counts that pin the form.
    // The high words that reach centre_rc (tests/test_partial_pairs.py proves both over the whole schedule):
    //   HI_FULL    the fold of a full-round layer: the rows of circ(2M4, M4, M4, M4) sum to at most 80, so V < 160 * 2^32;
    //   HI_PARTIAL word 0 after a single partial round or a pair (at most 165 492), and every word after a single round (at
    //              most 65 561): V < 2^50 with a small addend.
    static constexpr uint32_t HI_FULL = 160, HI_PARTIAL = 1u << 18;
    template <uint32_t RC, uint32_t HI>
    static __device__ __forceinline__ int32_t centre_rc(uint32_t t) {
        static_assert(HI < P - RC, "round constant too close to P for the fused reduction");
        constexpr uint32_t c = P - RC;
        static_assert((uint64_t)P + HI - c <= 0x7FFFFFFFull, "t - c leaves the int32 range");
        const int32_t a = (int32_t)(t - c);
        const uint32_t q = (uint32_t)(a >> 31) ^ 0xC0000000u;
        return (int32_t)((uint32_t)a + q);
    }

    template <int R, int I, int END = 16>
    static __device__ __forceinline__ void sbox_full(const uint64_t* V, uint32_t* s, const SboxK& k) {
        s[I] = pow5c(centre_rc<centred(RC_FULL_K[R][I]), HI_FULL>(fold2(V[I])), k);
        if constexpr (I + 1 < END) sbox_full<R, I + 1, END>(V, s, k);
    }
    // The linear layer and the S-box layer of round R behind it, ONE GROUP AT A TIME: the column sums (8 VGPRs) are live across
    // the layer with all sixteen input words, a group's z and M4 temporaries are about 8 more, and each of its four outputs
    // goes straight into its fold and S-box and replaces the group's input words — the whole V (32 VGPRs) never exists, and
    // the out-of-line instances stay within the 40 caller-saved registers.
    template <int R>
    static __device__ __forceinline__ void mds_sbox(uint32_t k2, uint32_t* s, const SboxK& k) {
        uint64_t X2[4], V[16];
        colsums_2x(k2, s, X2);
        mds_group_2x(k2, X2, s, V);           sbox_full<R, 0, 4>(V, s, k);
        mds_group_2x(k2, X2, s + 4, V + 4);   sbox_full<R, 4, 8>(V, s, k);
        mds_group_2x(k2, X2, s + 8, V + 8);   sbox_full<R, 8, 12>(V, s, k);
        mds_group_2x(k2, X2, s + 12, V + 12); sbox_full<R, 12, 16>(V, s, k);
    }
    // the layer alone, folded (<= P + HI_FULL): what the partial rounds take
    static __device__ __forceinline__ void mds_fold(uint32_t k2, uint32_t* s) {
        uint64_t X2[4];
        colsums_2x(k2, s, X2);
    #pragma unroll
        for (int g = 0; g < 4; g++) {
            uint64_t V[4];
            mds_group_2x(k2, X2, s + 4 * g, V);
    #pragma unroll
            for (int j = 0; j < 4; j++) s[4 * g + j] = fold2(V[j]);
        }
    }
    // the first full round of the second half takes its inputs already folded (from the last partial round, a single one)
    template <int I>
    static __device__ __forceinline__ void sbox_full4(uint32_t* s, const SboxK& k) {
        s[I] = pow5c(centre_rc<centred(RC_FULL_K[4][I]), HI_PARTIAL>(s[I]), k);
        if constexpr (I + 1 < 16) sbox_full4<I + 1>(s, k);
    }

    // Inputs: any u32 words, s[0] <= P + HI_PARTIAL.
    template <int R>
    static __device__ __forceinline__ void partial_round(uint32_t* s, uint32_t k2, uint32_t k6, const uint32_t* kd, const SboxK& k) {
        uint32_t u0 = pow5c(centre_rc<centred(RC_PARTIAL_K[R]), HI_PARTIAL>(s[0]), k);
        // sum2 = 2 * (u0 + s[1] + ... + s[15]) < 2^37, two chains
        uint64_t a = mul64(u0, k2), b = mul64(s[1], k2);
    #pragma unroll
        for (int i = 2; i < 16; i += 2) { a = mad64(s[i], k2, a); b = mad64(s[i + 1], k2, b); }
        uint64_t sum2 = add64(a, b);
        // 2 * (d_i * s_i + sum), d = (3, 4, 8, ..., 65536): < 2^50, so every fold is <= P + 2^18
        s[0] = fold2(mad64(u0, k6, sum2));
    #pragma unroll
        for (int i = 1; i < 16; i++) s[i] = fold2(mad64(s[i], kd[i], sum2));
    }

    // Partial rounds R and R + 1 in one pass.  With S = u0 + s_1 + ... + s_15 the sum of round R and d_i = 2^(i+1), round
    // R's words are s_i' = d_i s_i + S, and only word 0 of them is needed on its own (the next S-box input).  Round R + 1
    // takes the rest straight from round R's inputs:
    //     S'     = u0' + sum_i s_i' = u0' + sum_i d_i s_i + 15 S
    //     s_i''  = d_i s_i' + S'    = (d_i^2 mod P) s_i + d_i S + S'
    // so a word costs two multiply-accumulates and ONE fold over the pair instead of two and two.  kq[i] = 2 (d_i^2 mod P)
    // = 2^((2i + 2) mod 31 + 1), k30 = 2 * 15.  Inputs: any u32 words with s[0] <= P + HI_PARTIAL and s_14 < 2^32 - 2^24
    // (its multiplier is 2^31); tests/test_partial_pairs.py proves the bounds over the schedule.
    template <int R>
    static __device__ __forceinline__ void partial_pair(uint32_t* s, uint32_t k2, uint32_t k6, uint32_t k30, const uint32_t* kd,
                                                        const uint32_t* kq, const SboxK& k) {
        uint32_t u0 = pow5c(centre_rc<centred(RC_PARTIAL_K[R]), HI_PARTIAL>(s[0]), k);
        uint64_t a = mul64(u0, k2), b = mul64(s[1], k2);
    #pragma unroll
        for (int i = 2; i < 16; i += 2) { a = mad64(s[i], k2, a); b = mad64(s[i + 1], k2, b); }
        uint64_t sum2 = add64(a, b);                                          // 2S < 2^37
        const uint32_t s0 = fold2(mad64(u0, k6, sum2));                       // round R's word 0, <= P + 2^6
        const uint32_t sf = fold2(sum2);                                      // S, <= P + 2^5
        u0 = pow5c(centre_rc<centred(RC_PARTIAL_K[R + 1]), HI_PARTIAL>(s0), k);
        // sum2 = 2S' = 2 u0' + sum_i 2 d_i s_i + 30 S < 2^50 + 2^37, two chains
        a = mul64(u0, k2); b = mul64(s[1], kd[1]);
    #pragma unroll
        for (int i = 2; i < 16; i += 2) { a = mad64(s[i], kd[i], a); b = mad64(s[i + 1], kd[i + 1], b); }
        a = mad64(sf, k30, a);
        sum2 = add64(a, b);
        s[0] = fold2(mad64(u0, k6, sum2));                                    // <= P + HI_PARTIAL
        // 2 s_i'' < 2^63 (the largest term: 2^31 s_14), so the fold is exact
    #pragma unroll
        for (int i = 1; i < 16; i++) s[i] = fold2(mad64(s[i], kq[i], mad64(sf, kd[i], sum2)));
    }

    // Everything up to and including the S-box layer of the last full round: s = that layer's outputs (range L2).
    static __device__ __forceinline__ void poseidon2_rounds(uint32_t* s, uint32_t k2, uint32_t k4) {
        const uint32_t k6 = opaque(6);
        const SboxK k5 = sbox_k();
        // s: canonical input.  No accumulator carries a round constant: the constants are literals of the fused reductions.
        mds_sbox<0>(k2, s, k5);
        mds_sbox<1>(k2, s, k5);
        mds_sbox<2>(k2, s, k5);
        mds_sbox<3>(k2, s, k5);
        // partial rounds: every lane lazily folded (any u32 inside the pairs, <= P + 2^18 after a single round), lane 0 goes
        // through the S-box
        mds_fold(k2, s);
        // 2 * diag: 2^(i+2) for lanes 1..15, as opaque wave-uniform multipliers
        uint32_t kd[16];
        kd[0] = k6;
    #define RSV_KD(i) kd[i] = opaque(4u << (i));
        RSV_KD(1) RSV_KD(2) RSV_KD(3) RSV_KD(4) RSV_KD(5) RSV_KD(6) RSV_KD(7) RSV_KD(8)
        RSV_KD(9) RSV_KD(10) RSV_KD(11) RSV_KD(12) RSV_KD(13) RSV_KD(14) RSV_KD(15)
    #undef RSV_KD
        // 2 (d_i^2 mod P) = 2^(2i + 3) for lanes 1..14 (= kd[2i + 1] up to lane 7), 4 for lane 15
        uint32_t kq[16];
        kq[0] = 0;
    #pragma unroll
        for (int i = 1; i < 8; i++) kq[i] = kd[2 * i + 1];
    #define RSV_KQ(i) kq[i] = opaque(8u << (2 * (i)));
        RSV_KQ(8) RSV_KQ(9) RSV_KQ(10) RSV_KQ(11) RSV_KQ(12) RSV_KQ(13) RSV_KQ(14)
    #undef RSV_KQ
        kq[15] = k4;
        const uint32_t k30 = opaque(30);
        // 14 = 1 + 6 x 2 + 1.  The last round must be a single one: the pairs leave word 14 near 2^32 and word 13 above 2^31
        // (multipliers 2^31 and 2^29); a single round brings every word back to <= P + 2^18, within what sbox_full4 takes
        partial_round<0>(s, k2, k6, kd, k5);
        partial_pair<1>(s, k2, k6, k30, kd, kq, k5);  partial_pair<3>(s, k2, k6, k30, kd, kq, k5);  partial_pair<5>(s, k2, k6, k30, kd, kq, k5);
        partial_pair<7>(s, k2, k6, k30, kd, kq, k5);  partial_pair<9>(s, k2, k6, k30, kd, kq, k5);  partial_pair<11>(s, k2, k6, k30, kd, kq, k5);
        partial_round<13>(s, k2, k6, kd, k5);
        sbox_full4<0>(s, k5);
        mds_sbox<5>(k2, s, k5);
        mds_sbox<6>(k2, s, k5);
        mds_sbox<7>(k2, s, k5);
    }

    static __device__ __forceinline__ void poseidon2_inline(uint32_t* s) {
        const uint32_t k2 = opaque(2), k4 = opaque(4);
        poseidon2_rounds(s, k2, k4);
        mds_fold(k2, s);
        // canonical output: fold <= P + 160, so one conditional subtract lands in [0, P); P itself maps to 0
    #pragma unroll
        for (int i = 0; i < 16; i++) s[i] = min(s[i], s[i] - P);
    }

    // The last linear layer for ONE half of the state (HI false: words 0..7, the rate; true: words 8..15, the capacity): all
    // four column sums are needed either way, the z, the M4, the folds and the canonicalisations only for the two groups
    // asked for — every hash of the verify pipeline keeps one half of the permutation's output
    // (Poseidon2HalfVar::permute's ignore_left_result / ignore_right_result, primitives/poseidon31/src/lib.rs:251-288).
    // 16 + 8 multiplies and 2 x 8 v_lshl_add_u64.  The instance must fit the 40 caller-saved registers v0..v39 like
    // poseidon2(), or the Merkle kernels spill around every call.
    template <bool HI>
    static __device__ __forceinline__ void poseidon2_inline_half(uint32_t* s, uint32_t* out8) {
        const uint32_t k2 = opaque(2), k4 = opaque(4);
        poseidon2_rounds(s, k2, k4);
        uint64_t X2[4];
        colsums_2x(k2, s, X2);
    #pragma unroll
        for (int g = 0; g < 2; g++) {
            uint64_t V[4];
            mds_group_2x(k2, X2, s + (HI ? 8 : 0) + 4 * g, V);
    #pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t t = fold2(V[j]);
                out8[4 * g + j] = min(t, t - P);
            }
        }
    }
};
// (tools/perm_lab.hip, k_permute: the paced form)
__device__ __forceinline__ void poseidon2_inline(uint32_t* s) { PermT<true>::poseidon2_inline(s); }

#ifdef RSV_COUNT_PERMS
// Diagnostic build only (make count): executed permutations per kernel tag — [2t] active lanes, [2t+1] wave-level calls.
__device__ unsigned long long g_perm_counter[16];
__shared__ unsigned s_perm_tag;
#define RSV_TAG(k) do { if (threadIdx.x == 0) s_perm_tag = (k); __syncthreads(); } while (0)
// one wave-level call of an out-of-line instance, counted by the wave's first active lane
__device__ __forceinline__ void count_perm_call() {
    const unsigned long long m = __ballot(1);
    if ((threadIdx.x & 63u) == (unsigned)__builtin_ctzll(m)) {
        atomicAdd(&g_perm_counter[2 * (s_perm_tag & 7u)], (unsigned long long)__builtin_popcountll(m));
        atomicAdd(&g_perm_counter[2 * (s_perm_tag & 7u) + 1], 1ull);
    }
}
#else
#define RSV_TAG(k) do { } while (0)
__device__ __forceinline__ void count_perm_call() {}
#endif

// Out-of-line instance with the whole output state: rsv_poseidon2_permute*, the PoseidonFlow kernels.
__device__ __noinline__ State16 poseidon2(State16 st) {
    count_perm_call();
    poseidon2_inline(st.s);
    return st;
}

// Poseidon2HalfVar::permute semantics (primitives/poseidon31/src/lib.rs:282-311):
// state = left || right; returns rate = out[0..8] and capacity = out[8..16].
struct Hash8 {
    uint32_t w[8];
};
__device__ __forceinline__ State16 join(const Hash8& l, const Hash8& r) {
    State16 st;
#pragma unroll
    for (int i = 0; i < 8; i++) { st.s[i] = l.w[i]; st.s[8 + i] = r.w[i]; }
    return st;
}
__device__ __forceinline__ Hash8 rate_of(const State16& st) {
    Hash8 h;
#pragma unroll
    for (int i = 0; i < 8; i++) h.w[i] = st.s[i];
    return h;
}
__device__ __forceinline__ Hash8 cap_of(const State16& st) {
    Hash8 h;
#pragma unroll
    for (int i = 0; i < 8; i++) h.w[i] = st.s[8 + i];
    return h;
}
__device__ __forceinline__ Hash8 zero8() {
    Hash8 h;
#pragma unroll
    for (int i = 0; i < 8; i++) h.w[i] = 0;
    return h;
}
// (Until round 4 a second form stood beside this one — a single out-of-line instance with a run-time half selector, 51
// VGPRs, the Merkle kernels spilling 32 B per lane around its calls; same step time, 1 GB more traffic.  Its callers moved
// to the template arguments below, so it no longer compiled: removed.)
// One out-of-line instance per output half and pacing.  The Merkle kernels (several waves per SIMD wherever a launch
// fills the machine) call the PACED ones; the lane-form transcript — one wave per SIMD for 65 536 proofs — the unpaced
// ones (k_transcript: 3.21 -> 2.66 ms).  A choice per call site by launch size (tried: small batches' trees unpaced, one
// proof 1.31 -> 1.22 ms) doubles every call in the Merkle kernels, which then spill 80-112 bytes per lane around them and
// lose 4.7 % at 65 536 proofs: not taken; the choice is the call site's own template argument.
template <bool HI, bool PACE>
__device__ __noinline__ Hash8 poseidon2_half_t(State16 st) {
    count_perm_call();
    Hash8 h;
    PermT<PACE>::template poseidon2_inline_half<HI>(st.s, h.w);
    return h;
}
// The row form of the same call (poseidon2_row.hpp): the 16 lanes of a DPP row hold the SAME state and the same result,
// each computes one word of it.  For a launch of a few waves, where a lane-form permutation (one lane, sixteen words) is a
// chain of ~5 000 instructions and the row form one of ~1 250.
// Round constants of one lane: RC_FULL[r][i] for the eight full rounds, fetched ONCE per kernel (a load inside the
// round loop is consumed two instructions later and costs the wave its whole latency, eight times per permutation —
// more than the arithmetic of the round).  The partial-round constants are literals.
struct RowRC {
    uint32_t f[8];
};
__device__ __forceinline__ RowRC load_row_rc(uint32_t i) {
    RowRC k;
#pragma unroll
    for (int r = 0; r < 8; r++) k.f[r] = RC_FULL[r][i];
    return k;
}
template <bool HI>
__device__ __noinline__ Hash8 poseidon2_row_half(State16 st);
__device__ __noinline__ State16 poseidon2_row_state(State16 st);  // the whole output state (PoseidonFlow records)
// The row form's round constants for the out-of-line instance, in LDS: [round][lane of the row].  A kernel that calls
// poseidon2_half<FORM_ROW> fills the table first (row_rc_init).  Not global memory: a load inside the callee would make it
// wait for every load its caller has in flight (the memory counter is in order; LDS has a counter of its own) — the tree
// kernels fetch the next level's sibling while a level is hashed.  Not an argument either: eight more values live across
// every call, and the callers spill.
__shared__ uint32_t s_row_rc[8][16];
template <int PACE>
__device__ __forceinline__ void row_rc_init() {
    if constexpr (PACE == 2) {
        if (threadIdx.x < 128) s_row_rc[threadIdx.x >> 4][threadIdx.x & 15u] = RC_FULL[threadIdx.x >> 4][threadIdx.x & 15u];
        __syncthreads();
    }
}
// FORM (the `PACE` argument of every helper and kernel below and in merkle.hpp / k_merkle.hpp): 1 the paced lane form,
// 0 the unpaced lane form, 2 (FORM_ROW) the row form on "virtual lanes" of 16 lanes each.
constexpr int FORM_ROW = 2;
template <int PACE = 1>
__device__ __forceinline__ Hash8 poseidon2_half(State16 st, uint32_t hi) {  // hi is a literal at every call site
    if constexpr (PACE == FORM_ROW) return hi ? poseidon2_row_half<true>(st) : poseidon2_row_half<false>(st);
    else return hi ? poseidon2_half_t<true, PACE != 0>(st) : poseidon2_half_t<false, PACE != 0>(st);
}
// whole output state, by form (the PoseidonFlow kernels: lane form paced, or the row form)
template <int PACE = 1>
__device__ __forceinline__ State16 poseidon2_full(State16 st) {
    if constexpr (PACE == FORM_ROW) return poseidon2_row_state(st);
    else return poseidon2(st);
}
// the lane of a kernel's own indexing: a thread (lane forms) or a DPP row of 16 threads that all compute the same (row form)
template <int PACE>
__device__ __forceinline__ uint32_t vlane() { return PACE == FORM_ROW ? threadIdx.x >> 4 : threadIdx.x; }
template <int PACE = 1>
__device__ __forceinline__ Hash8 perm_rate(const Hash8& l, const Hash8& r) { return poseidon2_half<PACE>(join(l, r), 0u); }
template <int PACE = 1>
__device__ __forceinline__ Hash8 perm_cap(const Hash8& l, const Hash8& r) { return poseidon2_half<PACE>(join(l, r), 1u); }
__device__ __forceinline__ bool hash_eq(const Hash8& a, const Hash8& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a.w[i] ^ b.w[i];
    return d == 0;
}

}  // namespace rsv
