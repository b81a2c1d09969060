// k_pow.hpp — proof of work and queries of the next proof: the search for the nonce, the mix of the nonce found, and the
// draw of the query positions (pow_api.inc drives the launches; include/rsv.h: rsv_pow_grind_dev, rsv_draw_queries_dev).
// The semantics are the verifier's (k_transcript.hpp: the nonce split 22 / 21 / 21, one mix, pow_bits low zero bits of
// digest word 0, then ceil(n_queries / 8) draws).
#pragma once
#include "k_fri.hpp"

namespace rsv {

constexpr unsigned POW_BLOCK = 256;
constexpr uint64_t POW_NONE = ~0ull;  // best[p] before a nonce is found: no candidate reaches it (start + max_tries <= 2^64 - 1)

__device__ __forceinline__ Hash8 pow_rate(uint64_t nonce) {
    Hash8 l = zero8();
    l.w[0] = (uint32_t)(nonce & ((1u << 22) - 1));
    l.w[1] = (uint32_t)((nonce >> 22) & ((1u << 21) - 1));
    l.w[2] = (uint32_t)((nonce >> 43) & ((1u << 21) - 1));
    return l;
}

// ---------------------------------------------------------------- the search
// One lane per candidate, lane form: a candidate is one permutation (perm_cap: the rate half the nonce's three words, the
// capacity half the channel's digest) with nothing loaded or stored for it but the poll of best[p].  Grid row blockIdx.y
// is proof p0 + y; the lane with index g in its row tests start + g, start + g + stride, ... (stride = the row's lanes).
// A lane whose candidate qualifies lowers best[p] to it (64-bit atomicMin) and leaves on its next pass, as every lane does:
// before every candidate a lane reads best[p] (relaxed, device scope: served by L2, one 8-byte load per ~3 500 VALU
// instructions of the permutation, hidden behind the other waves of the SIMD) and leaves when best[p] is not above the
// candidate, or when the candidate reaches start + max_tries.  So best[p] ends as the SMALLEST qualifying nonce in
// [start, start + max_tries): a lane only ever skips candidates at or above a value best[p] held, and best[p] only
// falls.  A stale read delays an exit and nothing else; no lane waits for another, no loop is unbounded, and a workgroup
// that starts late finds best[p] below its first candidates and leaves at once — nothing depends on residency.
//
// GRID (pow_api.inc, pow_row_blocks): the lanes of a row are min(2^pow_bits, max_tries) rounded up to whole workgroups,
// at most what fills the machine once for the whole launch (8 workgroups of 256 per CU, shared among the rows), at
// least one workgroup.  The expected search is 2^pow_bits candidates, so a round of all lanes is never much more than
// that, and a small pow_bits does not pay for a machine-wide round.  OVER-SEARCH: beyond the nonce found, a row tests at
// most the rest of the round the hit lies in, plus the candidates that lanes running ahead of the hit's round have begun
// before the atomicMin is visible to them: about one round, i.e. the row's lanes (<= max(256, min(2^pow_bits, machine
// lanes))), against an expected 2^pow_bits to the hit.  Measured (profiles/HISTORY.md, "Proof of work and queries"): at
// 2^29.2 candidates to the hit, and for 16 proofs at 2^21 each, the search runs at the k_permute rate counted on the
// candidates up to the hit alone; the waves of a SIMD do not drift apart by more than the bound allows.
__global__ __launch_bounds__(POW_BLOCK) void k_pow_search(const uint32_t* __restrict__ chan, const uint8_t* __restrict__ ok, uint32_t p0,
                                                          uint32_t pow_bits, uint64_t start, uint64_t max_tries,
                                                          unsigned long long* __restrict__ best) {
    const uint32_t p = p0 + blockIdx.y;
    if (!ok[p]) return;
    const uint64_t stride = (uint64_t)gridDim.x * POW_BLOCK;
    const Hash8 digest = load_hash(chan + (size_t)p * 16);
    const uint32_t low = (1u << pow_bits) - 1u;
    unsigned long long* b = best + p;
    uint64_t t = (uint64_t)blockIdx.x * POW_BLOCK + threadIdx.x;  // the candidate's offset from start
#pragma unroll 1
    while (t < max_tries) {
        const uint64_t nonce = start + t;
        if (__hip_atomic_load(b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= nonce) break;
        const Hash8 d = perm_cap<1>(pow_rate(nonce), digest);
        // no break behind the hit: the next pass reads best[p] and leaves.  With a break here the compiler sinks the
        // atomic out of the loop, behind the exit of the wave's last lane: the minimum stayed unpublished until the hit's
        // wave had run out of candidates
        if ((d.w[0] & low) == 0u) atomicMin(b, (unsigned long long)nonce);
        if (max_tries - t <= stride) break;  // also keeps t from wrapping
        t += stride;
    }
}

// One lane per proof, after the search.  Found: the nonce to nonce [n][2] (low word first), mixed into chan [n][16]
// (digest, n_sent = 0).  Masked (ok[p] == 0) or exhausted (best[p] still POW_NONE; ok[p] is then cleared): zero nonce,
// zeroed channel, as the earlier stages leave a masked proof.
__global__ __launch_bounds__(64) void k_pow_finish(const unsigned long long* __restrict__ best, uint32_t n, uint8_t* __restrict__ ok,
                                                   uint32_t* __restrict__ chan, uint32_t* __restrict__ nonce) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    uint32_t* co = chan + (size_t)p * 16;
    const uint64_t found = best[p];
    if (!ok[p] || found == POW_NONE) {
        if (ok[p]) ok[p] = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) co[i] = 0u;
        nonce[2 * (size_t)p] = 0u;
        nonce[2 * (size_t)p + 1] = 0u;
        return;
    }
    Channel<0> ch;
    ch.init();
    ch.digest = load_hash(co);
    ch.mix(pow_rate(found));
    channel_store(co, ch);
    nonce[2 * (size_t)p] = (uint32_t)found;
    nonce[2 * (size_t)p + 1] = (uint32_t)(found >> 32);
}

// ---------------------------------------------------------------- the queries
// One lane per proof: ceil(nq / 8) draws from chan [n][16] (read and updated: n_sent moves on, the circuit's surplus
// draws are not made), each giving eight words in order, word k cut to its low log_size bits -> queries [n][nq]; low
// (may be nullptr) [n][nq]: the same positions >> (log_size - log_low).  A masked proof gets zeros and a zeroed channel.
__global__ __launch_bounds__(64) void k_pow_queries(const uint8_t* __restrict__ mask, uint32_t n, uint32_t nq, uint32_t log_size,
                                                    uint32_t log_low, uint32_t* __restrict__ chan, uint32_t* __restrict__ queries,
                                                    uint32_t* __restrict__ low) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    uint32_t* co = chan + (size_t)p * 16;
    uint32_t* qo = queries + (size_t)p * nq;
    uint32_t* lo = low ? low + (size_t)p * nq : nullptr;
    if (mask && !mask[p]) {
#pragma unroll
        for (int i = 0; i < 16; i++) co[i] = 0u;
        for (uint32_t i = 0; i < nq; i++) {
            qo[i] = 0u;
            if (lo) lo[i] = 0u;
        }
        return;
    }
    Channel<0> ch = channel_load(co);
    const uint32_t cut = (1u << log_size) - 1u, down = log_size - log_low;
#pragma unroll 1
    for (uint32_t got = 0; got < nq; got += 8) {
        const Hash8 d = ch.draw();
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            if (got + k < nq) {
                const uint32_t q = d.w[k] & cut;
                qo[got + k] = q;
                if (lo) lo[got + k] = q >> down;
            }
        }
    }
    co[8] = ch.n_sent;
}

}  // namespace rsv
