// k_pack.hpp — the next proof serialised on the device: the chain's buffers into the bytes of a PlonkWithPoseidonProof, in
// the verifier's blob layout (pack_api.inc drives the launches; include/rsv.h: rsv_proof_pack_dev).  The bytes are those of
// chain.proof_bytes (bincode: little-endian words, u64 length prefixes).
//
// A proof is R = 10 + 2 T runs (T layer trees), each a PREFIX of fixed length followed by a COPY of count * width words:
//   run 0 .. 3            hash_witness of trees 0 .. 3 (width 8).  Prefix of run 0: the fixed 895-word head, u64(4), the
//                         count; of the others: u64(0) (the column_witness of the tree before), the count.
//   run 4 .. 7            queried_values of trees 0 .. 3 (width 1).  Prefix of run 4: u64(0) (tree 3's column_witness),
//                         u64(4), the count; of the others: the count.
//   run 8 + 2 t           fri_witness of layer tree t (width 4).  Prefix: t = 0 the nonce's two words; t > 0 u64(0) (the
//                         column_witness of tree t - 1) and the eight words of its commitment, for t = 1 also u64(T - 1);
//                         then the count.
//   run 9 + 2 t           hash_witness of layer tree t (width 8).  Prefix: the count.
//   run 8 + 2 T           the last polynomial, 2^log_last values (width 4).  Prefix: u64(0), the commitment of tree T - 1,
//                         for T = 1 the u64(0) of the empty inner layers, u64(2^log_last).
//   run 9 + 2 T           nothing to copy.  Prefix: the word log_last, the proof's last.
// The prefixes of all runs are one MAP, the same for every proof of a call (pack_api.inc builds it on the host once per
// configuration): an entry is a literal word, the count of a run, or a word of one of the seven fixed-shape parts (sums,
// roots, root3, samples, samples3, nonce, fri_roots); pre_at[r] is where run r's prefix starts in it.  Every prefix has at
// least one word, so the runs' first output words begin[0] < begin[1] < ... are distinct.
//
//   k_pk_sizes   one wave per proof, a lane per run: the counts against their capacities and the mask, begin[p][0 .. R]
//                (a wave scan of the runs' words) and the length.
//   k_pk_scan    one workgroup: the exclusive scan of the lengths into d_offsets, 1 024 per step with a carry.
//   k_pk_pack    one lane per output word: the proof's begin table in LDS, a binary search for the word's run (at most 7
//                steps for R <= 68), then a map entry or a word of the run's source.  Consecutive lanes write consecutive
//                words and, within a run, read consecutive words; all accesses are dwords (a run starts anywhere).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace rsv {

constexpr uint32_t PK_HEAD = 895;                       // words before the decommitments
constexpr uint32_t PK_MAX_T = 29;                       // 1 + RSV_MAX_FRI_INNER
constexpr uint32_t PK_MAX_RUNS = 10 + 2 * PK_MAX_T;
constexpr uint32_t PK_SCAN = 1024;
// map entries (x: kind, y: value)
constexpr uint32_t PK_LIT = 0;   // the word y
constexpr uint32_t PK_CNT = 1;   // the count of run y (the low word of its u64 prefix)
constexpr uint32_t PK_SRC = 2;   // PK_SRC + k: word y of the proof's record in fixed part k
enum : uint32_t { PK_SUMS, PK_ROOTS, PK_ROOT3, PK_SAMPLES, PK_SAMPLES3, PK_NONCE, PK_FRI_ROOTS };

struct PkList {  // rsv_proof_list
    const uint32_t* items;
    uint64_t stride;
    const uint32_t* count;
    uint64_t count_stride;
    uint32_t cap;
};

struct PkArgs {
    PkList witness[4], values[4], fri_witness, fri_hash_witness;
    const uint32_t *sums, *roots, *root3, *samples, *samples3, *nonce, *fri_roots, *last_poly;
    const uint8_t* mask;      // may be null
    const uint2* map;
    const uint32_t* pre_at;   // [R + 1]
    uint32_t* begin;          // [n][R + 1]: the first output word of run r, begin[R] the proof's words
    uint64_t* len;            // [n] bytes
    uint32_t T, log_last;
};

struct PkRun {
    const uint32_t* items;
    const uint32_t* count;  // null: always `cap` items
    uint32_t cap, lw;       // lw: log2 of the item's words
};

__host__ __device__ constexpr uint32_t pk_runs(uint32_t T) { return 10 + 2 * T; }

__device__ __forceinline__ uint32_t pk_lw(uint32_t r, uint32_t T) {
    if (r < 4) return 3;
    if (r < 8) return 0;
    if (r < 8 + 2 * T) return r & 1 ? 3 : 2;
    return r == 8 + 2 * T ? 2 : 0;
}

__device__ __forceinline__ PkRun pk_of(const PkList& l, uint64_t p, uint32_t t, uint32_t lw) {
    return PkRun{l.items + p * l.stride + (((uint64_t)t * l.cap) << lw), l.count + p * l.count_stride + t, l.cap, lw};
}

// Run r of proof p.  The lists are named one by one: an index into the kernel's argument that is not a constant would put
// the whole argument into scratch.
__device__ __forceinline__ PkRun pk_run(const PkArgs& a, uint32_t r, uint64_t p) {
    if (r == 0) return pk_of(a.witness[0], p, 0, 3);
    if (r == 1) return pk_of(a.witness[1], p, 0, 3);
    if (r == 2) return pk_of(a.witness[2], p, 0, 3);
    if (r == 3) return pk_of(a.witness[3], p, 0, 3);
    if (r == 4) return pk_of(a.values[0], p, 0, 0);
    if (r == 5) return pk_of(a.values[1], p, 0, 0);
    if (r == 6) return pk_of(a.values[2], p, 0, 0);
    if (r == 7) return pk_of(a.values[3], p, 0, 0);
    if (r < 8 + 2 * a.T) return r & 1 ? pk_of(a.fri_hash_witness, p, (r - 8) >> 1, 3) : pk_of(a.fri_witness, p, (r - 8) >> 1, 2);
    if (r == 8 + 2 * a.T) return PkRun{a.last_poly + ((p * 4) << a.log_last), nullptr, 1u << a.log_last, 2};
    return PkRun{nullptr, nullptr, 0, 0};
}

__device__ __forceinline__ const uint32_t* pk_fixed(const PkArgs& a, uint32_t k, uint64_t p) {
    if (k == PK_SUMS) return a.sums + p * 8;
    if (k == PK_ROOTS) return a.roots + p * 24;
    if (k == PK_ROOT3) return a.root3 + p * 8;
    if (k == PK_SAMPLES) return a.samples + p * 536;
    if (k == PK_SAMPLES3) return a.samples3 + p * 32;
    if (k == PK_NONCE) return a.nonce + p * 2;
    return a.fri_roots + p * 8 * a.T;
}

// One wave per proof, a lane per run (two rounds past 64 runs): the run's words, a wave scan of them into begin[], the
// verdict by ballot.  (One lane per proof walking its 10 + 2 T runs is a chain of as many dependent loads: 16 us for one
// level-10 proof, more than the other two kernels together.)  A count above its capacity is clipped for the table (nothing
// is read past a capacity) and makes the proof's slot empty, as a cleared mask byte does.  The host has refused
// capacities whose proof exceeds 2^30 words.  Grid: n workgroups of 64.
__global__ __launch_bounds__(64) void k_pk_sizes(PkArgs a) {
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    const uint32_t R = pk_runs(a.T);
    uint32_t* begin = a.begin + (uint64_t)p * (R + 1);
    bool ok = true;
    uint32_t at = 0;
    for (uint32_t r0 = 0; r0 < R; r0 += 64) {
        const uint32_t r = r0 + lane;
        uint32_t words = 0;
        if (r < R) {
            const PkRun run = pk_run(a, r, p);
            uint32_t cnt = run.cap;
            if (run.count) {
                cnt = *run.count;
                if (cnt > run.cap) {
                    ok = false;
                    cnt = run.cap;
                }
            }
            words = a.pre_at[r + 1] - a.pre_at[r] + (cnt << run.lw);
        }
        uint32_t incl = words;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (r < R) begin[r] = at + incl - words;
        at += __shfl(incl, 63);
    }
    const bool all_ok = __ballot(!ok) == 0 && (!a.mask || a.mask[p]);
    if (lane == 0) {
        begin[R] = at;
        a.len[p] = all_ok ? (uint64_t)at * 4 : 0;
    }
}

// One workgroup (64 lanes for up to 64 proofs, else PK_SCAN): offsets[0] = 0, offsets[i + 1] = len[0] + ... + len[i], a
// workgroup's width of lengths per step (a Hillis-Steele scan between two LDS rows), the steps joined by a carry every
// lane holds.
__global__ __launch_bounds__(PK_SCAN) void k_pk_scan(const uint64_t* len, uint32_t n, uint64_t* offsets) {
    __shared__ uint64_t s[2][PK_SCAN];
    const uint32_t tid = threadIdx.x, width = blockDim.x;
    uint64_t carry = 0;
    if (tid == 0) offsets[0] = 0;
    for (uint32_t base = 0; base < n; base += width) {
        const uint32_t i = base + tid;
        uint32_t cur = 0;
        s[0][tid] = i < n ? len[i] : 0;
        __syncthreads();
        for (uint32_t d = 1; d < width; d <<= 1) {
            uint64_t x = s[cur][tid];
            if (tid >= d) x += s[cur][tid - d];
            cur ^= 1;
            s[cur][tid] = x;
            __syncthreads();
        }
        if (i < n) offsets[i + 1] = carry + s[cur][tid];
        carry += s[cur][width - 1];
        __syncthreads();  // the next step writes the rows again
    }
}

// Grid (256-word blocks of the longest possible proof, proofs p0 .. of this launch).  A proof is written iff it ends within
// blob_cap; the blocks past a proof's words, and all blocks of an empty slot, leave at once.
__global__ __launch_bounds__(256) void k_pk_pack(PkArgs a, uint32_t p0, const uint64_t* offsets, uint32_t* blob, uint64_t blob_cap) {
    __shared__ uint32_t s_begin[PK_MAX_RUNS + 1], s_pre[PK_MAX_RUNS + 1];
    __shared__ const uint32_t* s_src[PK_MAX_RUNS];
    const uint32_t p = p0 + blockIdx.y;
    const uint64_t o0 = offsets[p], o1 = offsets[p + 1];
    const uint32_t words = (uint32_t)((o1 - o0) >> 2);
    if (o1 > blob_cap || blockIdx.x * 256 >= words) return;
    const uint32_t R = pk_runs(a.T);
    for (uint32_t r = threadIdx.x; r <= R; r += 256) {
        s_begin[r] = a.begin[(uint64_t)p * (R + 1) + r];
        s_pre[r] = a.pre_at[r];
        if (r < R) s_src[r] = pk_run(a, r, p).items;
    }
    __syncthreads();
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    uint32_t lo = 0, hi = R;  // the run of word w: the last r with begin[r] <= w
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_begin[mid] <= w) lo = mid;
        else hi = mid;
    }
    const uint32_t off = w - s_begin[lo], pre = s_pre[lo], pre_len = s_pre[lo + 1] - pre;
    uint32_t v;
    if (off >= pre_len) {
        v = s_src[lo][off - pre_len];
    } else {
        const uint2 e = a.map[pre + off];
        if (e.x == PK_LIT) v = e.y;
        else if (e.x == PK_CNT) v = (s_begin[e.y + 1] - s_begin[e.y] - (s_pre[e.y + 1] - s_pre[e.y])) >> pk_lw(e.y, a.T);
        else v = pk_fixed(a, e.x - PK_SRC, p)[e.y];
    }
    blob[(o0 >> 2) + w] = v;
}

}  // namespace rsv
