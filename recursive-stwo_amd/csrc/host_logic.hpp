// host_logic.hpp — the HOST-side decisions of a verify call that touch no device: how a mixed batch is bucketed by
// shape, how the per-query stages are cut into groups that fit the workspace budget, which form of every kernel a batch
// runs and on which stream (VerifyPlan: plan_batch before the groups are known, plan_launches and plan_group after), and
// (plan_pass) how a stage of the next proof sizes a pass of proofs and blocks to that budget.  Plain C++ (no HIP): included by
// verify_api.inc, and compiled on its own by g++ with AddressSanitizer + UBSan for tests/host_logic_asan.cpp, which drives
// it from recorded and adversarial shape arrays and pins the plan of every batch size at which a form changes — the host
// code of the mixed-batch path had never seen a sanitizer before round 4 (the r3a crash pointed at exactly
// this code or at the test's own threads).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <new>
#include <stdexcept>
#include <unordered_map>
#include <vector>

#include "../../include/rsv.h"
#include "layout.hpp"
#include "options.hpp"

namespace rsv::host {

// workspace carving: 256-byte aligned sub-allocations of one buffer (base == nullptr: size probe)
struct Carve {
    char* base;
    size_t off = 0;
    template <class T> T* take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += sizeof(T) * count;
        return p;
    }
};

// The offsets of a batch as the host-pointer forms stage them (host_stage.inc): rel[i] = offsets[i] - offsets[0] for
// i = 0 .. n, so that proof 0 starts at byte 0 of the staged blob.  RSV_E_SIZE exactly when some offsets[i + 1] < offsets[i].
inline int rebase_offsets(const uint64_t* offsets, size_t n, std::vector<uint64_t>& rel) {
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return RSV_E_SIZE;
    try {
        rel.resize(n + 1);
    } catch (const std::bad_alloc&) {
        return RSV_E_NOMEM;
    } catch (const std::length_error&) {
        return RSV_E_NOMEM;
    }
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - offsets[0];
    return RSV_OK;
}

// One launch geometry: every proof of a bucket has n_queries = G.  maxM / maxInner / minLevel bound its trees.
struct Bucket { uint32_t G, maxM, maxInner, minLevel, count; size_t first; };

// The parser's two shape words per proof (k_parse.hpp): word0 = n_queries | M << 8 | n_inner << 16 | min level << 24 (0: the
// proof was rejected, no lane anywhere), word1 = the tree geometry.  Mixed batch: one bucket per n_queries; inside a bucket
// the slots are ordered by shape class, so that the lanes of a wavefront (and nearly every workgroup) walk trees of one
// geometry.  ids: slot -> proof.  cls / scratch: caller-owned (reused call after call).
inline void bucket_by_shape(const uint32_t* shape, uint32_t N, std::vector<Bucket>& buckets, std::vector<uint32_t>& ids,
                            std::vector<uint32_t>& cls) {
    struct Class { uint32_t w0, w1, count; size_t start; };
    std::vector<Class> classes;
    std::unordered_map<uint64_t, uint32_t> class_of;  // hashed lookup: an adversarial batch may carry thousands of distinct shapes
    buckets.clear();
    cls.resize(N);
    uint32_t last_w0 = 0, last_w1 = 0, last_c = 0;
    for (uint32_t p = 0; p < N; p++) {
        const uint32_t w0 = shape[2 * (size_t)p], w1 = shape[2 * (size_t)p + 1];
        if (!w0) { cls[p] = 0xFFFFFFFFu; continue; }
        uint32_t ci;
        if (!classes.empty() && w0 == last_w0 && w1 == last_w1) ci = last_c;
        else {
            auto it = class_of.find(((uint64_t)w0 << 32) | w1);
            if (it != class_of.end()) ci = it->second;
            else {
                ci = (uint32_t)classes.size();
                class_of.emplace(((uint64_t)w0 << 32) | w1, ci);
                classes.push_back({w0, w1, 0, 0});
            }
            last_w0 = w0; last_w1 = w1; last_c = ci;
        }
        cls[p] = ci;
        classes[ci].count++;
    }
    // class order: by n_queries, then by the shape words
    std::vector<uint32_t> order(classes.size());
    for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const Class &a = classes[x], &b = classes[y];
        if ((a.w0 & 0xFFu) != (b.w0 & 0xFFu)) return (a.w0 & 0xFFu) < (b.w0 & 0xFFu);
        if (a.w0 != b.w0) return a.w0 < b.w0;
        return a.w1 < b.w1;
    });
    size_t at = 0;
    for (uint32_t ci : order) {
        Class& c2 = classes[ci];
        c2.start = at;
        at += c2.count;
        const uint32_t q = c2.w0 & 0xFFu;
        if (buckets.empty() || buckets.back().G != q) buckets.push_back({q, 0, 0, 255, 0, c2.start});
        Bucket& b = buckets.back();
        b.maxM = std::max(b.maxM, (c2.w0 >> 8) & 0xFFu);
        b.maxInner = std::max(b.maxInner, (c2.w0 >> 16) & 0xFFu);
        b.minLevel = std::min(b.minLevel, c2.w0 >> 24);
        b.count += c2.count;
    }
    ids.resize(at);
    std::vector<size_t> fill(classes.size());
    for (size_t i = 0; i < classes.size(); i++) fill[i] = classes[i].start;
    for (uint32_t p = 0; p < N; p++)
        if (cls[p] != 0xFFFFFFFFu) ids[fill[cls[p]]++] = p;
}

// One (bucket, slot range) of a group: cn slots of bucket bi from slot c0 on, launched with G lanes per proof, the dense
// top-of-tree cap from level Lc down.  Lt: the level at which the tree kernels hand their nodes over to the cap kernels
// (0: the whole cap inside the tree kernels); Lt2 <= Lt: the level from which k_cap_top (one lane per tree) walks to the
// root; the levels between Lt and Lt2 belong to k_cap_mid (one lane per subtree).
struct Entry { size_t bi; size_t c0; uint32_t cn, G, Lc, Lt, Lt2; size_t bytes; };

struct GroupPolicy {
    size_t budget;         // bytes of per-query workspace a group may use
    size_t max_fused;      // entries per launch (Fused<>)
    bool tree_cap_off;     // RSV_OPT_TREE_CAP = 2
    bool flow;             // the pass writes PoseidonFlow records
    bool flow_cap_off;     // RSV_OPT_FLOW_CAP = 2
    bool cap_top;          // the last levels of the cap in k_cap_top
    int cap_mid = 0;       // RSV_OPT_CAP_MID: 0 by the fill of the in-kernel cap levels, 1 hand over at the cap level wherever the cap kernels can take it, 2 never
};

// lanes per proof of a bucket's launches: tiny query counts are padded so that a workgroup holds at most 64 proofs
inline uint32_t padded_lanes(const Bucket& b) { return b.G < 4 ? 4u : b.G; }

// Cap levels of a bucket.  Lc: 2^Lc <= G, strictly below every tree's lowest leaf / data level (0: no cap).  Inside the
// tree kernels a cap level l keeps (proofs per workgroup) x 2^l lanes busy, each part-filled wave at the price of a full
// wave-level permutation: 16-query proofs (16 per workgroup) fill whole waves at levels 3 and 2 and leave only the last
// two levels to k_cap_top (Lt = Lt2 = 2); three 80-query proofs put 96, 48 and 24 lanes into 2 + 1 + 1 waves (256 slots
// for 168 nodes), nine 27-query proofs 72 and 36 lanes into 2 + 1 waves, 25 ten-query proofs 100 lanes into 2.  Such a
// bucket hands its level-Lc nodes over (Lt = Lc) and the cap kernels, whose lanes are dealt over the whole launch, take
// it from there: k_cap_mid a subtree per lane down to level Lt2, k_cap_top the rest (k_merkle.hpp).
// hand-over at the cap level: k_cap_top holds 2^Lt2 <= 8 nodes in registers, k_cap_mid walks Lt - Lt2 = 2 or 3 levels
inline void handover_levels(uint32_t Lc, uint32_t& Lt, uint32_t& Lt2) {
    Lt = Lc;
    Lt2 = Lc <= 3 ? Lc : (Lc >= 6 ? 3u : 2u);
}
inline void cap_levels(const Bucket& b, const GroupPolicy& pol, uint32_t block, uint32_t& Lc, uint32_t& Lt, uint32_t& Lt2) {
    const uint32_t G = padded_lanes(b);
    Lc = 0;
    while ((2u << Lc) <= G) Lc++;
    if (b.minLevel < 2) Lc = 0;
    else if (Lc > b.minLevel - 1) Lc = b.minLevel - 1;
    if (Lc > 6) Lc = 6;
    if (Lc < 2) Lc = 0;
    if (pol.tree_cap_off) Lc = 0;
    if (pol.flow && pol.flow_cap_off) Lc = 0;  // every lane walks (and records) its whole path
    Lt = Lt2 = (pol.cap_top && !pol.flow && Lc >= 3) ? (Lc >= 6 ? 3u : 2u) : 0u;  // the cap kernels write no records
    if (!Lt || pol.cap_mid == 2) return;
    // wave slots of the in-kernel cap levels against the nodes they hold
    const uint32_t pb = std::min<uint32_t>(block / G, 64u);
    uint32_t slots = 0, nodes = 0;
    for (uint32_t l = Lt; l < Lc; l++) { slots += ((pb << l) + 63u) / 64u * 64u; nodes += pb << l; }
    if (pol.cap_mid == 1 || slots * 100u > nodes * 115u) handover_levels(Lc, Lt, Lt2);
}

// per-query workspace of cn slots of a bucket (what verify_impl carves for one Entry)
inline size_t entry_bytes(const Bucket& b, uint32_t G, size_t cn, uint32_t Lt, uint32_t Lt2) {
    Carve probe{nullptr};
    probe.take<PlanHdr>(cn);
    probe.take<uint32_t>(cn * (b.maxM + 1) * G);
    probe.take<uint32_t>(cn * 2 * G);
    probe.take<uint32_t>(cn * (3 + b.maxInner) * G * 8);
    for (uint32_t L : {Lt, Lt2 != Lt ? Lt2 : 0u})
        if (L) {
            probe.take<uint32_t>((cn * 4 << L) * 8);
            probe.take<unsigned long long>(cn * 4);
            probe.take<uint32_t>((cn * (1 + b.maxInner) << L) * 8);
            probe.take<unsigned long long>(cn * (1 + b.maxInner));
        }
    return ((probe.off + 255) & ~(size_t)255) + 256;
}

// The batch is cut into GROUPS of at most max_fused entries whose workspaces fit the budget together; a group is ONE launch
// per stage.  A uniform batch is one entry (several groups only when it exceeds the budget), a mixed batch normally one
// group with an entry per n_queries.  Returns the workspace bytes the largest group needs.
inline size_t plan_groups(const std::vector<Bucket>& buckets, const GroupPolicy& pol, std::vector<std::vector<Entry>>& groups) {
    groups.clear();
    size_t need = 0;
    std::vector<Entry> cur;
    size_t used = 0;
    auto flush = [&]() { if (!cur.empty()) { groups.push_back(cur); need = std::max(need, used); cur.clear(); used = 0; } };
    // widest buckets first: their workgroups are the longest-running, and a launch's tail should be short ones
    for (size_t bk = buckets.size(); bk-- > 0;) {
        const size_t bi = bk;
        const Bucket& b = buckets[bi];
        const uint32_t G = padded_lanes(b);
        uint32_t Lc, Lt, Lt2;
        cap_levels(b, pol, 256u, Lc, Lt, Lt2);
        const size_t per_slot = entry_bytes(b, G, 1024, Lt, Lt2) / 1024 + 1;
        for (size_t c0 = 0; c0 < b.count;) {
            size_t room = pol.budget > used ? (pol.budget - used) / per_slot : 0;
            size_t cn = std::min<size_t>(b.count - c0, room);
            if (cn < std::min<size_t>(b.count - c0, 1024)) {  // not worth a sliver: start a new group
                if (!cur.empty()) { flush(); continue; }
                cn = std::min<size_t>(b.count - c0, 1024);       // a budget below 1 024 slots: take them anyway
            }
            Entry en{bi, c0, (uint32_t)cn, G, Lc, Lt, Lt2, entry_bytes(b, G, cn, Lt, Lt2)};
            cur.push_back(en);
            used += en.bytes;
            c0 += cn;
            if (cur.size() == pol.max_fused) flush();
        }
    }
    flush();
    return need;
}

// ---------------------------------------------------------------- the launch plan of a verify call
// Every form decision of verify_impl (verify_api.inc) depends only on the batch size, the configuration, the options and the
// outputs asked for.  They are taken here, in two steps — plan_batch before the groups are known, plan_launches (and
// plan_group, per group) after — and the launcher only reads the result.

constexpr int kBlock = 256;
// Row form of the tree kernels (k_merkle.hpp): 512 threads = 32 virtual lanes per workgroup (two waves per SIMD: 256 registers); chosen while the FRI-tree
// launch holds at most this many paths (proofs x queries x trees).
constexpr int kRowTreeBlock = 512;
constexpr uint64_t kRowTreeLanes = 256ull * 16 * 9;
constexpr uint64_t kRowQueryLanes = 256ull * 16;  // k_query's row form: up to this many queries (proofs x queries) in the launch

// what a verify call is asked for, as far as a form depends on it
struct PlanInputs {
    uint32_t N;                              // proofs of the batch
    uint32_t n_cfgs;                         // the configuration set: how many, ...
    bool cfg_of;                             // ... whether every proof names its own, ...
    uint32_t log_blowup, log_last, n_queries;  // ... and configuration 0
    bool flow;                               // the pass writes PoseidonFlow records
    bool paths;                              // outputs indexed by one declared shape (PathsOut::paths)
    bool trace_sib, pair_sib;                // sibling outputs of the trace trees / of the FRI trees
    bool own;                                // every proof has its own public inputs
    size_t max_fused;                        // entries per launch (Fused<>)
};

struct VerifyPlan {
    // plan_batch
    bool transcript_row, transcript_split, transcript_paced;
    bool device_order;   // slot order on the device, nothing read back
    int tree_form;       // the PACE / FORM template argument of the tree kernels: 1 paced, 0 unpaced, 2 row
    bool small_trees;    // the row hashes on the unpaced permutation instances
    bool qconst_row, qconst4;
    bool oods_row;
    bool cap_top;
    bool serial_plan;    // one-lane-per-proof original (tests)
    bool pair_deal;      // the FRI trees of a small launch dealt out over the compute units (pair_layer_order)
    GroupPolicy policy;
    // plan_launches
    uint32_t tree_lanes;  // lanes of the tree kernels' indexing per workgroup
    bool overlap_trees, chain, query_row, qconst_in_plan;
    bool oods_on_main;    // the OODS kernel inside the one group, on the main stream; else last on the side stream
};

// the OODS evaluation has a lane form and a row form
// small batches: one proof per 16-lane row (latency form); large ones: one proof per lane (throughput form).
// RSV_OPT_OODS_FORM overrides (tests).  The row form is a latency form: it pays while the kernel is on the step's chain
// of dependent kernels; since it runs behind the trace trees beside k_pair_merkle (and costs three times the issue slots
// per proof) the lane form wins from 8 192 proofs on (4 096: 2.82 vs 2.97 ms; 8 192: 5.43 vs 5.38; 16 384: 10.31 vs
// 10.14; 24 576: 15.09 vs 14.67).
inline bool oods_row_form(const Options& o, size_t n) { return o.oods_form ? o.oods_form == 1 : n <= 6144; }

inline VerifyPlan plan_batch(const Options& o, const PlanInputs& in) {
    VerifyPlan p{};
    const uint32_t N = in.N;
    // small batches: one proof per 16-lane DPP row (latency form of the transcript); large ones: one proof per lane
    // (throughput form).  RSV_OPT_TRANSCRIPT_FORM overrides (tests).
    // measured crossover on MI355X: 16 384 proofs 1.41 M/s (row) vs 1.26 M/s (lane), 32 768: 1.32 vs 1.36
    p.transcript_row = o.transcript_form ? o.transcript_form == 1 : N <= 24576;
    // Up to one wave per SIMD (4 096 proofs) the row form runs as two launches: the front half needs nothing from the
    // parser and starts next to it on the aux stream (k_transcript.hpp): 1 024 proofs 1.67 -> 1.63 ms, 4 096 2.89 -> 2.82;
    // at 8 192 it is a wash and beyond that the two halves and the parser get in each other's way (12 288: +12 %).
    // RSV_OPT_TRANSCRIPT_SPLIT overrides (tests).  The lane form (large batches) always runs as one launch (split the same
    // way, it measured 35.46 vs 35.20 ms at 65 536 proofs: inside run-to-run noise), and so does a pass that writes the flow.
    p.transcript_split = p.transcript_row && !in.flow && (o.transcript_split ? o.transcript_split == 2 : N <= 4096);
    // the lane form without flow: up to one wave per SIMD on the unpaced channel (k_transcript.hpp)
    p.transcript_paced = !p.transcript_row && !in.flow && N > 49152;
    // A batch under ONE configuration is one launch geometry of known size (n_queries is the configuration's, every
    // proof either carries it or is rejected by the parser): nothing has to come back to the host.  The slot order by
    // shape class is made on the device (k_parse.hpp) and the tables are sized for the largest trees the parser lets
    // through, so the call enqueues everything and returns: no host synchronisation anywhere in it.  Batches under
    // several configurations (several n_queries buckets whose sizes only the device knows) and calls with per-query path
    // outputs (one declared shape, checked on the host) keep the round trip of rounds 1-2.
    p.device_order = in.n_cfgs == 1 && !in.cfg_of && !in.paths && o.device_order != 2 && in.n_queries >= 1 && in.n_queries <= (uint32_t)MAXQ &&
                     in.log_blowup >= 1 && in.log_blowup <= 16 && in.log_last <= 16;
    // A batch whose FRI-tree launch puts fewer than about two and a half waves on a SIMD (at most 1 024 proofs of 16 queries
    // and nine trees; measured: one proof 1.31 -> 1.21 ms, 512 proofs 1.43 -> 1.34, 768: 1.45 -> 1.35, 1 024: 1.467 -> 1.457,
    // 2 048: 1.906 -> 1.945, slower) runs the
    // tree kernels on the unpaced permutation instances.  An estimate from the configuration (the batch's real depth is on
    // the device only): proofs x queries x (FRI trees of the common depth M = 22).
    // Up to 256 proofs of 16 queries the trees go one step further, to the ROW form on virtual lanes (k_merkle.hpp): 16 threads per
    // path, every permutation shared by a DPP row.  RSV_OPT_TREE_PACE overrides (1 paced, 2 unpaced, 3 row).
    const uint32_t nq_est = in.n_queries < 4 ? 4u : in.n_queries, fold_est = in.log_blowup + in.log_last;
    const uint64_t lanes = (uint64_t)N * nq_est * (22u > fold_est ? 22u - fold_est : 1u);
    p.tree_form = 1;
    if (o.tree_pace) p.tree_form = o.tree_pace == 1 ? 1 : (o.tree_pace == 2 ? 0 : 2);
    else if (in.n_cfgs == 1 && lanes <= kRowTreeLanes) p.tree_form = 2;
    else if (in.n_cfgs == 1 && lanes <= 1024ull * 16 * 9) p.tree_form = 0;
    if (in.flow && p.tree_form == 0) p.tree_form = 1;  // (the FLOW instantiations: paced lane form and row form)
    // a small batch's launches leave a wave nearly alone on its SIMD: the unpaced permutation instances (poseidon2.hpp)
    p.small_trees = p.tree_form != 1;  // (the row hashes: lane forms only; they run underneath the transcript)
    // the quotient constants, small batches: one proof per 16-lane row (latency form); RSV_OPT_QCONST_FORM overrides (tests)
    p.qconst_row = o.qconst_form ? o.qconst_form == 1 : N <= 24576;
    // the row form of the quotient constants on four rows per proof (k_plan.hpp: qconst_row_body); RSV_OPT_QCONST_FORM = 1
    // forces the row form with ONE row per proof (what batches of 4 097 .. 24 576 proofs run), so that tests reach it
    p.qconst4 = N <= 4096 && o.qconst_form != 1;
    p.oods_row = oods_row_form(o, N);
    // The top of the cap in its own kernel (k_cap_top: one lane per tree instead of a part-filled wave per workgroup):
    // fewer permutation slots, two more launches — from 1 024 proofs on (measured: 1 024 proofs 1.663 -> 1.652 ms, 16 384: 9.98 -> 9.84, 65 536: 34.96 -> 34.37; a single proof would wait for three sequential hashes of a 17-lane launch),
    // and not while per-query paths are emitted (the cap writes the top of every path as it goes).
    p.cap_top = !(in.trace_sib || in.pair_sib) && (o.cap_top ? o.cap_top == 1 : N >= 1024);
    p.serial_plan = o.plan_form == 2;
    p.pair_deal = o.pair_order != 2;
    p.policy = GroupPolicy{(size_t)o.ws_budget_mb << 20, in.max_fused, o.tree_cap == 2, in.flow, o.flow_cap == 2, p.cap_top, o.cap_mid};
    return p;
}

// Step two: what depends on how plan_groups cut the batch.
inline void plan_launches(VerifyPlan& p, const Options& o, const PlanInputs& in, const std::vector<std::vector<Entry>>& groups) {
    bool wide = false;  // an entry with more queries than a workgroup of the row forms has virtual lanes
    for (const std::vector<Entry>& grp : groups)
        for (const Entry& en : grp) wide = wide || en.G > (uint32_t)kRowTreeBlock / 16u;
    if (p.tree_form == 2 && wide) p.tree_form = in.flow ? 1 : 0;
    p.tree_lanes = p.tree_form == 2 ? (uint32_t)kRowTreeBlock / 16u : (uint32_t)kBlock;
    // The FRI trees go to the SIDE stream right behind k_query (the only thing they wait for) and run next to the
    // trace trees instead of after them; the two kernels that only feed k_finalize (OODS check, canonicity scan)
    // follow the trace trees on the main stream.  A small batch leaves most of the chip idle and its step is a
    // chain of dependent kernels, so the overlap shortens it (1 024 proofs -3 %, 2 048 -4 %, 8 192 -2.4 %); a
    // large one fills the chip with either kernel and gains 0.4 % (65 536 proofs: 35.7 vs 35.9 ms).  Batches cut
    // into several groups keep the serial order: the groups share one workspace.
    p.overlap_trees = groups.size() == 1 && o.overlap_trees != 2;
    // Stream layout of a single-group batch.  "Chain" (RSV_OPT_CRITICAL_CHAIN): every kernel the verdict waits for
    // longest sits on ONE stream, in order — transcript, quotient constants, plan, k_query, FRI trees, finalize — and
    // the side stream takes what finishes early anyway (row hashes, then — behind the plan — trace trees and the OODS
    // check).  A kernel that waits for another stream's event starts ~20 us after it (measured on MI355X: 18-28 us
    // against 5-11 us behind a kernel of its own stream); the two-stream layout of rounds 1-2 had three such waits
    // on the path of a small batch (transcript -> k_qconst, k_plan -> k_query, FRI trees -> finalize).
    // measured: +1..4 % from 512 to 16 384 proofs, -2 % at 32 768 and beyond
    p.chain = p.overlap_trees && (o.critical_chain ? o.critical_chain == 1 : in.N <= 24576);
    // k_query on virtual lanes (k_query.hpp: 16 threads per query split its sums): RSV_OPT_QUERY_FORM, or by size
    p.query_row = p.chain && !wide &&
                  (o.query_form ? o.query_form == 1 : (uint64_t)in.N * (in.n_queries < 4 ? 4u : in.n_queries) <= kRowQueryLanes && in.n_cfgs == 1);
    // the row-form quotient constants of a chain-layout batch ride in the plan's launch (k_plan_par<.., true>)
    p.qconst_in_plan = p.chain && !p.serial_plan && p.qconst_row;
    // The OODS composition check only raises failure flags (atomicOr) for k_finalize.  Single-group batch outside the chain
    // layout: on the main stream in front of the trace trees' last levels, which wait for the FRI trees to leave them room —
    // so it runs underneath the FRI trees, not behind them.  Else last on the side stream (chain: behind the trace trees;
    // several groups: behind k_query).
    p.oods_on_main = p.overlap_trees && !p.chain;
}

struct GroupPlan {
    bool tm_t, tm_p;         // item order of the cap kernels over the trace / FRI trees: tree-major
    size_t pair_lds;         // dynamic LDS of k_pair_merkle
    uint32_t group_M, live;  // the weights of pair_layer_order: tree depth, grid rows that have work
};

inline GroupPlan plan_group(const VerifyPlan& p, const PlanInputs& in, const std::vector<Bucket>& buckets, const std::vector<Entry>& grp) {
    GroupPlan g{};
    uint64_t top_t = 0, top_p = 0;  // workgroups of k_cap_top over the trace / FRI trees
    uint32_t max_inner = 0;
    for (const Entry& en : grp) {
        const Bucket& b = buckets[en.bi];
        top_t += ((uint64_t)en.cn * 4 + 255) / 256;
        top_p += ((uint64_t)en.cn * (1 + b.maxInner) + 255) / 256;
        max_inner = std::max(max_inner, b.maxInner);
        g.group_M = std::max(g.group_M, b.maxM);
    }
    // item order of the cap kernels (k_merkle.hpp: CapTopIndex): tree-major for launches of >= 2^19 lanes
    g.tm_t = top_t * 256 >= (1u << 19);
    g.tm_p = top_p * 256 >= (1u << 19);
    g.pair_lds = (in.pair_sib || in.flow) ? (size_t)kBlock * 32 : 0;
    g.live = 1 + max_inner;
    if (p.device_order) {
        // the launch is sized for MAX_LOG; what the batch really holds is on the device only.  The weights assume
        // the common depth of the reference's proofs (M = 22): a batch of deeper or shallower trees is still dealt
        // out better than row y = tree y, and any order is a correct one.
        g.group_M = 22;
        const uint32_t fold = in.log_blowup + in.log_last;
        g.live = g.group_M > fold ? g.group_M - fold : 1u;
    }
    return g;
}

// One pass of a stage that streams the next proof's column groups (commit_api.inc): P proofs times nb blocks.
struct Pass { size_t P, nb; };

// The largest pass whose workspace bytes(P, nb) fits the budget: all max_nb blocks of all n proofs, then fewer blocks
// (halved, rounded up, down to one), then fewer proofs; {1, 1} where nothing fits.  A stage without blocks passes 1.
template <class Bytes>
Pass plan_pass(size_t budget, size_t n, size_t max_nb, Bytes bytes) {
    Pass p{n, max_nb};
    while (p.nb > 1 && bytes(p.P, p.nb) > budget) p.nb = (p.nb + 1) / 2;
    while (p.P > 1 && bytes(p.P, p.nb) > budget) p.P = (p.P + 1) / 2;
    return p;
}

// Which FRI tree each grid row (blockIdx.y) of a SMALL k_pair_merkle launch hashes.  A launch whose workgroups are all
// resident at once is not balanced by the dispatcher: workgroup i lands on compute unit i mod n_cu (round robin over the
// XCDs, then inside them), so with `blocks` workgroups per grid row the rows pile up on the same compute units — 1 024
// proofs of the standard shape are 64 x 9 workgroups: the first 64 compute units get rows 0, 4 and 8 (the first-layer tree
// and two more: 67 path steps per SIMD), the others two rows (40-44), and the kernel lasts as long as the fullest.  The
// trees differ in depth (first layer M + columns, inner layer i: M - 1 - i), so the host deals them out: compute units
// that receive more rows get the shallowest trees, the rest longest-first onto the least loaded (LPT).  Identity when
// the launch is larger than the machine holds (the dispatcher then balances by itself, longest trees first).
// live: grid rows that have work (a single-configuration launch is sized for the deepest tree the parser admits, MAX_LOG: its
// rows beyond the batch's real FRI layers exit at once and weigh nothing).
inline void pair_layer_order(uint32_t blocks, uint32_t layers, uint32_t live, uint32_t M, uint32_t n_cu, uint32_t resident_per_cu, uint8_t* y_of) {
    for (uint32_t k = 0; k < 32; k++) y_of[k] = (uint8_t)k;
    if (live > layers) live = layers;
    if (layers < 3 || live < 3 || layers > 32 || blocks == 0 || n_cu == 0 || (size_t)blocks * live > (size_t)n_cu * resident_per_cu || blocks >= n_cu) return;
    // path steps of tree y (relative weights are what matters)
    std::vector<uint32_t> len(layers);
    for (uint32_t y = 0; y < layers; y++) len[y] = y >= live ? 0u : (y == 0 ? M + 8 : (M > y ? M - y : 1) + 4);
    // rows per compute unit, and the compute units each grid position covers
    std::vector<uint32_t> rows_of_cu(n_cu, 0), load(n_cu, 0);
    auto first_cu = [&](uint32_t pos) { return (uint32_t)(((size_t)pos * blocks) % n_cu); };
    for (uint32_t pos = 0; pos < layers; pos++)
        for (uint32_t x = 0; x < blocks; x++) rows_of_cu[(first_cu(pos) + x) % n_cu]++;
    std::vector<uint8_t> pos_used(layers, 0), tree_used(layers, 0);
    std::vector<uint32_t> by_len(layers);
    for (uint32_t y = 0; y < layers; y++) by_len[y] = y;
    std::sort(by_len.begin(), by_len.end(), [&](uint32_t a, uint32_t b) { return len[a] != len[b] ? len[a] > len[b] : a < b; });  // longest first
    auto assign = [&](uint32_t pos, uint32_t tree) {
        y_of[pos] = (uint8_t)tree; pos_used[pos] = 1; tree_used[tree] = 1;
        for (uint32_t x = 0; x < blocks; x++) load[(first_cu(pos) + x) % n_cu] += len[tree];
    };
    auto max_rows = [&](uint32_t pos) { uint32_t m = 0; for (uint32_t x = 0; x < blocks; x++) m = std::max(m, rows_of_cu[(first_cu(pos) + x) % n_cu]); return m; };
    uint32_t min_rows = 0xFFFFFFFFu;
    for (uint32_t c = 0; c < n_cu; c++) if (rows_of_cu[c]) min_rows = std::min(min_rows, rows_of_cu[c]);
    // phase A: positions over compute units with more rows than the others take the shallowest trees, one per surplus row
    std::vector<uint32_t> surplus_taken(n_cu, 0);
    for (uint32_t pos = layers; pos-- > 0;) {
        const uint32_t c0 = first_cu(pos);
        if (max_rows(pos) > min_rows && surplus_taken[c0] + min_rows < rows_of_cu[c0]) {
            uint32_t tree = 0xFFFFFFFFu;
            for (uint32_t k = layers; k-- > 0;) if (!tree_used[by_len[k]]) { tree = by_len[k]; break; }  // shallowest left
            assign(pos, tree);
            for (uint32_t x = 0; x < blocks; x++) surplus_taken[(c0 + x) % n_cu]++;
        }
    }
    // phase B: the rest longest-first onto the free position whose compute units carry least
    for (uint32_t k = 0; k < layers; k++) {
        const uint32_t tree = by_len[k];
        if (tree_used[tree]) continue;
        uint32_t best = 0xFFFFFFFFu, best_load = 0xFFFFFFFFu;
        for (uint32_t pos = 0; pos < layers; pos++) {
            if (pos_used[pos]) continue;
            uint32_t m = 0;
            for (uint32_t x = 0; x < blocks; x++) m = std::max(m, load[(first_cu(pos) + x) % n_cu]);
            if (m < best_load) { best_load = m; best = pos; }
        }
        assign(best, tree);
    }
}

}  // namespace rsv::host
