// host_logic_asan.cpp — TEST INFRASTRUCTURE: the product's host-only logic under AddressSanitizer + UBSan, in the CPU
// container (no HIP, no device, g++).  Built and driven by tests/test_host_logic_asan.py.
//
//   host_logic_asan program <hints file> <out file>   circuit_program.hpp: parse_template + build_program (the C++ mirror of
//                                                     the reference's gadgets, ~1 400 lines) on hints recorded on the CPU, then
//                                                     check_program on the result and on mutated copies of it; the program is
//                                                     written out for comparison with the Python restatement's
//   host_logic_asan buckets <seed> <rounds>           host_logic.hpp: bucket_by_shape + plan_groups on seeded shape arrays —
//                                                     recorded fixture shapes, garbage, thousands of distinct shapes, rejected
//                                                     proofs, 1 .. 128 queries — with the invariants the launcher relies on
//   host_logic_asan passes <seed> <rounds>            host_logic.hpp: plan_pass on seeded workspace costs, monotone in the proofs
//                                                     and the blocks of a pass — block counts that are powers of two and that
//                                                     are not, budgets from below the smallest pass to above the largest —
//                                                     against the two loops every streaming driver used to carry
//   host_logic_asan plan                              host_logic.hpp: the launch plan of a verify call (plan_batch, plan_launches,
//                                                     plan_group), one line per case over every batch size at which a form
//                                                     changes, for comparison with the restatement of what the launcher
//                                                     used to decide inline (tests/verify_plan_ref.py)
//   host_logic_asan offsets <seed> <rounds>          host_logic.hpp: rebase_offsets, which every host-pointer batch form stages its
//                                                     offsets through, on seeded offset arrays in exact-size heap copies — 0 to a
//                                                     few thousand proofs, base 0 and not, equal neighbours, one decreasing pair at
//                                                     every position of a short array, offsets near 2^63 — against the property:
//                                                     rel[i] == offsets[i] - offsets[0], or RSV_E_SIZE exactly when a pair decreases
//
// The hints file: 16 header words (magic, proof bytes, nq, M, n_inner, flow_count, n_pi, copies, 0...), then the proof
// (padded to words), trace_sib, trace_pos, trace_cols, fri_sib, fri_cols, flow [flow_count][32], swap (bytes, padded),
// public inputs [n_pi][5], set_walks (bytes, padded).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../recursive-stwo_amd/csrc/host_logic.hpp"
#include "../recursive-stwo_amd/csrc/circuit_program.hpp"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

using namespace rsv;

static std::vector<uint32_t> read_words(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f);
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    CHECK(n > 0 && n % 4 == 0);
    std::vector<uint32_t> w((size_t)n / 4);
    CHECK(fread(w.data(), 4, w.size(), f) == w.size());
    fclose(f);
    return w;
}

static int run_program(const char* in_path, const char* out_path) {
    const std::vector<uint32_t> file = read_words(in_path);
    CHECK(file.size() > 16 && file[0] == 0x52535648u);
    const size_t len = file[1], nq = file[2], M = file[3], n_inner = file[4], flow_count = file[5], n_pi = file[6], copies = file[7];
    const size_t nt = 1 + n_inner;
    size_t at = 16;
    auto take = [&](size_t words) { const uint32_t* p = file.data() + at; at += words; CHECK(at <= file.size()); return p; };
    const uint32_t* proof_w = take((len + 3) / 4);
    const uint32_t* trace_sib = take(4 * nq * M * 8);
    const uint32_t* trace_pos = take(4 * nq);
    const uint32_t* trace_cols = take(4 * nq * 64);
    const uint32_t* fri_sib = take(nt * nq * M * 8);
    const uint32_t* fri_cols = take(nt * nq * 24);
    const uint32_t* flow = take(flow_count * 32);
    const uint8_t* swap = reinterpret_cast<const uint8_t*>(take((flow_count + 3) / 4));
    const uint32_t* pi = take(n_pi * 5);
    const uint8_t* walks = reinterpret_cast<const uint8_t*>(take((copies + 3) / 4));
    CHECK(at == file.size());
    // exact-size heap copies, so that the sanitizer sees every read past an array's end
    std::vector<uint32_t> v_tsib(trace_sib, trace_sib + 4 * nq * M * 8), v_tpos(trace_pos, trace_pos + 4 * nq),
        v_tcols(trace_cols, trace_cols + 4 * nq * 64), v_fsib(fri_sib, fri_sib + nt * nq * M * 8), v_fcols(fri_cols, fri_cols + nt * nq * 24),
        v_flow(flow, flow + flow_count * 32), v_proof(proof_w, proof_w + (len + 3) / 4);
    std::vector<uint8_t> v_swap(swap, swap + flow_count), v_walks(walks, walks + copies);

    circuit::Template d{};
    const uint8_t* proof = reinterpret_cast<const uint8_t*>(v_proof.data());
    CHECK(circuit::parse_template(proof, len, d) == RSV_OK);
    CHECK(d.nq == nq && d.M == M && d.n_inner == n_inner);
    // malformed templates are refused, never read out of bounds: every truncation, a misaligned buffer, absurd header words
    for (size_t cut : {(size_t)0, (size_t)4, (size_t)64, len / 2, len - 4, len - 1}) {
        std::vector<uint8_t> part(proof, proof + cut);
        circuit::Template t{};
        CHECK(circuit::parse_template(part.data(), cut, t) != RSV_OK || cut == len);
    }
    {
        std::vector<uint8_t> shifted(len + 8);
        memcpy(shifted.data() + 1, proof, len);
        circuit::Template t{};
        CHECK(circuit::parse_template(shifted.data() + 1, len, t) == RSV_E_SIZE);
        for (uint32_t word : {0u, 1u, 10u, 11u, 12u, 13u}) {
            std::vector<uint32_t> bad(v_proof);
            bad[word] = 0xFFFFFFFFu;
            circuit::Template t2{};
            (void)circuit::parse_template(reinterpret_cast<const uint8_t*>(bad.data()), len, t2);  // any status, no bad access
        }
    }
    d.trace_sib = v_tsib.data(); d.trace_pos = v_tpos.data(); d.trace_cols = v_tcols.data();
    d.fri_sib = v_fsib.data(); d.fri_cols = v_fcols.data();
    std::vector<std::pair<uint32_t, circuit::Q4>> inputs;
    for (size_t i = 0; i < n_pi; i++) inputs.push_back({pi[5 * i], circuit::Q4{pi[5 * i + 1], pi[5 * i + 2], pi[5 * i + 3], pi[5 * i + 4]}});
    circuit::BuiltProgram bp;
    CHECK(circuit::build_program(d, v_flow.data(), v_swap.data(), (uint32_t)flow_count, inputs, (uint32_t)copies, v_walks.data(), bp) == RSV_OK);
    // hints that do not belong to the template make the gadgets' own checks fail: an error status, never a crash
    {
        std::vector<uint32_t> bad_flow(v_flow);
        bad_flow[bad_flow.size() / 2] ^= 1;
        circuit::BuiltProgram b2;
        CHECK(circuit::build_program(d, bad_flow.data(), v_swap.data(), (uint32_t)flow_count, inputs, (uint32_t)copies, v_walks.data(), b2) == RSV_E_RANGE);
        circuit::BuiltProgram b3;  // a flow that is too short for the circuit
        CHECK(circuit::build_program(d, v_flow.data(), v_swap.data(), (uint32_t)flow_count - 1, inputs, (uint32_t)copies, v_walks.data(), b3) == RSV_E_RANGE);
    }
    const size_t n_levels = bp.level_offsets.size() - 1;
    rsv_witness_shape shape{d.lp, d.lq, d.pow_bits, d.blowup, d.log_last, d.nq, d.n_inner, (uint32_t)flow_count, (uint32_t)copies};
    CHECK(circuit::check_program(bp.instr.data(), bp.n_vars, bp.level_offsets.data(), n_levels, (uint32_t)bp.n_vars, shape) == RSV_OK);
    // mutated programs: every field of seeded instructions pushed out of range, the level table broken
    std::mt19937 rng(7);
    size_t refused = 0, tried = 0;
    for (int k = 0; k < 400; k++) {
        std::vector<uint32_t> bad(bp.instr);
        const size_t i = rng() % bp.n_vars;
        const int field = (int)(rng() % 8);
        const uint32_t vals[] = {0xFFFFFFFFu, (uint32_t)bp.n_vars, (uint32_t)bp.n_vars + 1, 0x7FFFFFFFu, 64u, 1u << 20};
        bad[i * 8 + field] = vals[rng() % 6];
        const int rc = circuit::check_program(bad.data(), bp.n_vars, bp.level_offsets.data(), n_levels, (uint32_t)bp.n_vars, shape);
        tried++;
        refused += rc != RSV_OK;
        // an opcode or a destination out of range is ALWAYS refused (an operand or an immediate may be unused by the op)
        if (field <= 1 && bad[i * 8 + field] >= bp.n_vars) CHECK(rc != RSV_OK);
    }
    CHECK(refused >= tried / 8);
    {
        std::vector<uint32_t> lv(bp.level_offsets);
        lv[n_levels / 2] = lv[n_levels / 2 + 1] + 1;  // not monotone
        CHECK(circuit::check_program(bp.instr.data(), bp.n_vars, lv.data(), n_levels, (uint32_t)bp.n_vars, shape) != RSV_OK);
        lv = bp.level_offsets;
        lv[n_levels] += 1;                             // does not cover the program
        CHECK(circuit::check_program(bp.instr.data(), bp.n_vars, lv.data(), n_levels, (uint32_t)bp.n_vars, shape) != RSV_OK);
        rsv_witness_shape s2 = shape;
        s2.n_queries = 3;
        CHECK(circuit::check_program(bp.instr.data(), bp.n_vars, bp.level_offsets.data(), n_levels, (uint32_t)bp.n_vars, s2) != RSV_OK);
    }
    FILE* f = fopen(out_path, "wb");
    CHECK(f);
    const uint32_t hdr[8] = {0x52535650u, (uint32_t)bp.n_vars, (uint32_t)n_levels, (uint32_t)bp.flow_wires.size(), (uint32_t)bp.gates.size(),
                             (uint32_t)bp.witness_ops.size(), 0, 0};
    fwrite(hdr, 4, 8, f);
    fwrite(bp.instr.data(), 4, bp.instr.size(), f);
    fwrite(bp.level_offsets.data(), 4, bp.level_offsets.size(), f);
    fwrite(bp.flow_wires.data(), 4, bp.flow_wires.size(), f);
    fwrite(bp.gates.data(), 4, bp.gates.size(), f);
    fwrite(bp.witness_ops.data(), 4, bp.witness_ops.size(), f);
    fclose(f);
    printf("program: %zu variables, %zu levels, %zu rows, %zu of %zu mutated programs refused\n", bp.n_vars, n_levels, bp.gates.size() / 6,
           refused, tried);
    return 0;
}

// shape word 0 of a proof as k_parse writes it
static uint32_t w0_of(uint32_t nq, uint32_t M, uint32_t n_inner, uint32_t min_level) { return nq | (M << 8) | (n_inner << 16) | (min_level << 24); }

static void check_buckets(const std::vector<uint32_t>& shape, uint32_t N, size_t budget, size_t max_fused, bool cap_top) {
    std::vector<host::Bucket> buckets;
    std::vector<uint32_t> ids, cls;
    host::bucket_by_shape(shape.data(), N, buckets, ids, cls);
    // ids: every live proof exactly once; buckets: a partition of the slots by n_queries, ascending, bounds of their members
    size_t live = 0;
    for (uint32_t p = 0; p < N; p++) live += shape[2 * (size_t)p] != 0;
    CHECK(ids.size() == live && cls.size() == N);
    std::vector<uint8_t> seen(N, 0);
    for (uint32_t p : ids) { CHECK(p < N && !seen[p] && shape[2 * (size_t)p] != 0); seen[p] = 1; }
    size_t at = 0;
    uint32_t prev_g = 0;
    for (const host::Bucket& b : buckets) {
        CHECK(b.first == at && b.count > 0 && b.G > prev_g);
        prev_g = b.G;
        for (size_t s = b.first; s < b.first + b.count; s++) {
            const uint32_t w0 = shape[2 * (size_t)ids[s]];
            CHECK((w0 & 0xFFu) == b.G && ((w0 >> 8) & 0xFFu) <= b.maxM && ((w0 >> 16) & 0xFFu) <= b.maxInner && (w0 >> 24) >= b.minLevel);
            if (s > b.first) {  // inside a bucket: slots ordered by shape class
                const uint32_t q0 = shape[2 * (size_t)ids[s - 1]], q1 = shape[2 * (size_t)ids[s - 1] + 1];
                CHECK(q0 < w0 || (q0 == w0 && q1 <= shape[2 * (size_t)ids[s] + 1]));
            }
        }
        at += b.count;
    }
    CHECK(at == live);
    // groups: every slot of every bucket in exactly one entry; a group within the budget unless it is a single minimum entry
    std::vector<std::vector<host::Entry>> groups;
    const host::GroupPolicy pol{budget, max_fused, false, false, false, cap_top, (int)((N + budget) % 3)};  // RSV_OPT_CAP_MID: every setting over the runs
    const size_t need = host::plan_groups(buckets, pol, groups);
    std::vector<std::vector<std::pair<size_t, size_t>>> ranges(buckets.size());
    size_t worst = 0;
    for (const auto& g : groups) {
        CHECK(!g.empty() && g.size() <= max_fused);
        size_t used = 0;
        for (const host::Entry& e : g) {
            CHECK(e.bi < buckets.size() && e.cn > 0 && e.c0 + e.cn <= buckets[e.bi].count);
            CHECK(e.G >= 4 && e.G >= buckets[e.bi].G && e.Lc <= 6 && e.Lt <= e.Lc && e.Lt2 <= 3 && e.Lt2 <= e.Lt && e.Lt - e.Lt2 <= 3 && (e.Lt - e.Lt2 != 1) && (e.Lt == 0 || (e.Lc >= 3 && e.Lt2 >= 2)));
            CHECK(e.bytes == host::entry_bytes(buckets[e.bi], e.G, e.cn, e.Lt, e.Lt2));
            ranges[e.bi].push_back({e.c0, e.cn});
            used += e.bytes;
        }
        CHECK(used <= budget || g.size() == 1 || g.back().cn <= 1024);
        worst = std::max(worst, used);
    }
    for (size_t bi = 0; bi < buckets.size(); bi++) {  // every slot of every bucket in exactly one entry
        std::sort(ranges[bi].begin(), ranges[bi].end());
        size_t at = 0;
        for (auto& r : ranges[bi]) { CHECK(r.first == at); at += r.second; }
        CHECK(at == buckets[bi].count);
    }
    CHECK(need == worst);
}

static int run_buckets(uint32_t seed, int rounds) {
    std::mt19937 rng(seed);
    // the shapes of the reference's fixtures (n_queries, M, n_inner, min level) as the parser reports them
    const uint32_t fixtures[][4] = {{16, 21, 10, 8}, {16, 22, 8, 14}, {16, 23, 9, 14}, {80, 21, 12, 10}, {27, 21, 10, 12}, {11, 25, 10, 16},
                                    {10, 26, 10, 17}, {8, 27, 10, 17}, {8, 28, 11, 17}};
    for (int r = 0; r < rounds; r++) {
        const uint32_t N = r == 0 ? 1 : (r == 1 ? 53248 : 1 + rng() % 20000);
        std::vector<uint32_t> shape(2 * (size_t)N);
        const int mode = r % 5;
        for (uint32_t p = 0; p < N; p++) {
            uint32_t w0, w1;
            if (mode == 0 || mode == 1) {  // the recursion chain's mix, some proofs rejected by the parser
                const uint32_t* f = fixtures[(mode == 1 ? p / 4096 : rng()) % 9];
                w0 = w0_of(f[0], f[1], f[2], f[3]);
                w1 = f[1] * 1000 + f[2];
                if (rng() % 17 == 0) w0 = 0;
            } else if (mode == 2) {        // adversarial: (almost) every proof its own shape
                w0 = w0_of(1 + rng() % 128, 1 + rng() % 30, rng() % 29, rng() % 30);
                w1 = rng();
            } else if (mode == 3) {        // everything rejected, or one survivor
                w0 = (p == N / 2 && (r & 8)) ? w0_of(128, 30, 28, 2) : 0;
                w1 = 0;
            } else {                       // tiny query counts (padded to 4 lanes), minimum levels around the cap's threshold
                w0 = w0_of(1 + rng() % 6, 5 + rng() % 6, rng() % 4, rng() % 5);
                w1 = rng() % 3;
            }
            shape[2 * (size_t)p] = w0;
            shape[2 * (size_t)p + 1] = w1;
        }
        const size_t budgets[] = {(size_t)1 << 20, (size_t)512 << 20, (size_t)8192 << 20};
        check_buckets(shape, N, budgets[r % 3], r % 2 ? 16 : 3, (r & 4) != 0);
    }
    printf("buckets: %d rounds, invariants hold\n", rounds);
    return 0;
}

// A workspace as the streaming drivers carve it (Carve: every part rounded up to 256 bytes): a fixed part, parts per
// proof, per block and per (proof, block), and one that never falls below a word.  Monotone in P and in nb.
struct PassCost {
    size_t fixed, per_proof, per_block, per_both, leaves;
    size_t operator()(size_t P, size_t nb) const {
        host::Carve sz{nullptr};
        sz.take<uint32_t>(fixed);
        sz.take<uint32_t>(P * per_proof);
        sz.take<uint32_t>(nb * per_block);
        sz.take<uint32_t>(P * nb * per_both);
        sz.take<uint32_t>(std::max<size_t>(P * nb * leaves / 2, 1));
        return sz.off;
    }
};

static int run_passes(uint32_t seed, int rounds) {
    std::mt19937 rng(seed);
    const size_t block_counts[] = {1, 2, 4, 16, 256, 3, 27, 80};
    size_t cut_blocks = 0, cut_proofs = 0, whole = 0, floor = 0;
    for (int r = 0; r < rounds; r++) {
        const size_t n = r % 7 == 0 ? 1 : 1 + rng() % (r % 3 ? 40 : 5000), max_nb = block_counts[r % 8];
        const PassCost cost{rng() % 4096, rng() % 512, rng() % 2048, 1 + rng() % 65536, rng() % 64};
        const size_t lo = cost(1, 1), hi = cost(n, max_nb);
        CHECK(lo <= hi);
        // below the smallest pass, each end exactly and one byte either side, above the largest pass, seeded points between
        std::vector<size_t> budgets = {0, lo / 2, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, 2 * hi, cost(n, 1) - 1, cost(n, 1), cost(1, max_nb)};
        for (int k = 0; k < 24; k++) budgets.push_back(lo + (size_t)(((uint64_t)rng() << 32 | rng()) % (hi - lo + 1)));
        for (const size_t budget : budgets) {
            size_t calls = 0;
            const host::Pass got = host::plan_pass(budget, n, max_nb, [&](size_t P, size_t nb) {
                CHECK(P >= 1 && P <= n && nb >= 1 && nb <= max_nb);
                calls++;
                return cost(P, nb);
            });
            // the two loops as the drivers wrote them
            size_t P = n, nb = max_nb;
            while (cost(P, nb) > budget && nb > 1) nb = (nb + 1) / 2;
            while (cost(P, nb) > budget && P > 1) P = (P + 1) / 2;
            CHECK(got.P == P && got.nb == nb);
            CHECK(cost(got.P, got.nb) <= budget || (got.P == 1 && got.nb == 1));
            if (hi <= budget) CHECK(got.P == n && got.nb == max_nb);
            if (cost(n, 1) <= budget) CHECK(got.P == n);  // monotone: some nb fits at P == n exactly when nb == 1 does
            CHECK(calls <= 2 + 8 + 13);                   // a probe per halving: log2 of 256 blocks, of 5000 proofs
            whole += got.P == n && got.nb == max_nb;
            cut_blocks += got.nb < max_nb;
            cut_proofs += got.P < n;
            floor += cost(got.P, got.nb) > budget;
        }
    }
    CHECK(rounds < 16 || (whole && cut_blocks && cut_proofs && floor));  // every outcome was met
    printf("passes: %d rounds, invariants hold (%zu whole, %zu fewer blocks, %zu fewer proofs, %zu over budget at (1, 1))\n", rounds, whole,
           cut_blocks, cut_proofs, floor);
    return 0;
}

// The launch plan of a verify call (host_logic.hpp: plan_batch, plan_launches, plan_group) over the full product of batch
// sizes, configurations, requested outputs, options (one at a time away from its default) and sets of group entries: one
// line per case, the case first, then every field of both steps and of every group.  tests/test_host_logic_asan.py holds
// the same product and compares each line with tests/verify_plan_ref.py.
static int run_plan() {
    const uint32_t Ns[] = {1, 256, 257, 1023, 1024, 1025, 2048, 4096, 4097, 6144, 6145, 8192, 24576, 24577, 49152, 49153, 65536};
    const uint32_t queries[] = {1, 3, 4, 16, 32, 33, 80, 128};
    const uint32_t folds[][2] = {{1, 0}, {1, 16}, {4, 3}, {16, 0}, {16, 16}};  // (log_blowup, log_last)
    struct IntOpt { const char* name; int Options::*field; int max; };
    const IntOpt int_opts[] = {{"transcript_form", &Options::transcript_form, 2}, {"transcript_split", &Options::transcript_split, 2},
                               {"oods_form", &Options::oods_form, 2}, {"qconst_form", &Options::qconst_form, 2}, {"plan_form", &Options::plan_form, 2},
                               {"tree_cap", &Options::tree_cap, 2}, {"overlap_trees", &Options::overlap_trees, 2},
                               {"critical_chain", &Options::critical_chain, 2}, {"device_order", &Options::device_order, 2},
                               {"flow_cap", &Options::flow_cap, 2}, {"query_form", &Options::query_form, 2}, {"tree_pace", &Options::tree_pace, 3},
                               {"pair_order", &Options::pair_order, 2}, {"cap_mid", &Options::cap_mid, 2}, {"cap_top", &Options::cap_top, 2}};
    const long long budgets_mb[] = {1, 512, 1ll << 20};  // RSV_OPT_WS_BUDGET_MB: both ends of its range and one between
    struct Setting { const char* name; long long value; Options o; };
    std::vector<Setting> settings;
    settings.push_back({"default", 0, Options{}});
    for (const IntOpt& io : int_opts)
        for (int val = 1; val <= io.max; val++) {
            Options o;
            o.*io.field = val;
            settings.push_back({io.name, val, o});
        }
    for (long long mb : budgets_mb) {
        Options o;
        o.ws_budget_mb = mb;
        settings.push_back({"ws_budget_mb", mb, o});
    }
    size_t cases = 0;
    for (uint32_t N : Ns) {
    // the three sets of group entries.  0: one entry of G = 16;  1: one entry of G = 33;  2: two groups, the first of two entries
    const std::vector<host::Bucket> bucket_sets[3] = {{{16, 22, 10, 8, N, 0}}, {{33, 21, 9, 8, N, 0}}, {{16, 22, 10, 8, 2 * N, 0}, {27, 24, 12, 8, 3 * N, 2 * (size_t)N}}};
    const std::vector<std::vector<host::Entry>> group_sets[3] = {
        {{host::Entry{0, 0, N, 16, 0, 0, 0, 0}}}, {{host::Entry{0, 0, N, 33, 0, 0, 0, 0}}},
        {{host::Entry{0, 0, N, 16, 0, 0, 0, 0}, host::Entry{1, 0, 3 * N, 27, 0, 0, 0, 0}}, {host::Entry{0, N, N, 16, 0, 0, 0, 0}}}};
    for (uint32_t nq : queries) for (const auto& fold : folds) for (int cfg_mode = 0; cfg_mode < 3; cfg_mode++)
    for (int flow = 0; flow < 2; flow++) for (int paths = 0; paths < 2; paths++) for (int sib = 0; sib < 3; sib++) for (int own = 0; own < 2; own++)
    for (const Setting& s : settings) {
        // cfg_mode: 0 one configuration, 1 two, 2 one with cfg_of set;  sib: 0 none, 1 the trace trees', 2 the FRI trees'
        const host::PlanInputs in{N, cfg_mode == 1 ? 2u : 1u, cfg_mode == 2, fold[0], fold[1], nq, flow != 0, paths != 0, sib == 1, sib == 2, own != 0, 16};
        const host::VerifyPlan one = host::plan_batch(s.o, in);
        for (int gset = 0; gset < 3; gset++) {
            const std::vector<host::Bucket>& buckets = bucket_sets[gset];
            const std::vector<std::vector<host::Entry>>& groups = group_sets[gset];
            host::VerifyPlan p = one;
            host::plan_launches(p, s.o, in, groups);
            printf("%u %u %u %u %d %d %d %d %d %s %lld %d :", N, nq, fold[0], fold[1], cfg_mode, flow, paths, sib, own, s.name, s.value, gset);
            printf(" %d %d %d %d %d %d %d %d %d %d %d %d", one.transcript_row, one.transcript_split, one.transcript_paced, one.device_order, one.tree_form,
                   one.small_trees, one.qconst_row, one.qconst4, one.oods_row, one.cap_top, one.serial_plan, one.pair_deal);
            printf(" %zu %zu %d %d %d %d %d :", one.policy.budget, one.policy.max_fused, one.policy.tree_cap_off, one.policy.flow, one.policy.flow_cap_off,
                   one.policy.cap_top, one.policy.cap_mid);
            printf(" %d %u %d %d %d %d %d", p.tree_form, p.tree_lanes, p.overlap_trees, p.chain, p.query_row, p.qconst_in_plan, p.oods_on_main);
            for (const auto& grp : groups) {
                const host::GroupPlan g = host::plan_group(p, in, buckets, grp);
                printf(" : %d %d %zu %u %u", g.tm_t, g.tm_p, g.pair_lds, g.group_M, g.live);
            }
            printf("\n");
            cases++;
        }
    }
    }
    fprintf(stderr, "plan: %zu cases\n", cases);
    return 0;
}

// rel[i] == offsets[i] - offsets[0] for i = 0 .. n, or RSV_E_SIZE exactly when some offsets[i + 1] < offsets[i]
static void check_rebase(const std::vector<uint64_t>& offsets, size_t& refused) {
    const size_t n = offsets.size() - 1;
    bool decreases = false;
    for (size_t i = 0; i < n; i++) decreases |= offsets[i + 1] < offsets[i];
    std::vector<uint64_t> rel(3, 0xDEADu);  // (whatever it held is replaced)
    const int rc = host::rebase_offsets(offsets.data(), n, rel);
    CHECK(rc == (decreases ? RSV_E_SIZE : RSV_OK));
    refused += decreases;
    if (decreases) return;
    CHECK(rel.size() == n + 1);
    for (size_t i = 0; i <= n; i++) CHECK(rel[i] == offsets[i] - offsets[0]);
}

static int run_offsets(uint32_t seed, int rounds) {
    std::mt19937_64 rng(seed);
    size_t cases = 0, refused = 0;
    const uint64_t bases[] = {0, 7, 1ull << 32, (1ull << 63) - (1ull << 40), 1ull << 63};
    for (int r = 0; r < rounds; r++) {
        const size_t n = r < 4 ? (size_t)r : (r % 5 == 0 ? 2000 + rng() % 3000 : rng() % 64);
        std::vector<uint64_t> offsets(n + 1);  // exact size: a read of offsets[n + 1] is a heap overflow
        offsets[0] = bases[r % 5];
        const uint64_t step = r % 3 == 0 ? 1 : (r % 3 == 1 ? 500000 : 1ull << 36);
        for (size_t i = 0; i < n; i++) offsets[i + 1] = offsets[i] + (rng() % 4 == 0 ? 0 : rng() % step);  // a quarter of the neighbours equal
        check_rebase(offsets, refused);
        cases++;
    }
    // one decreasing pair at every position of a short array, at every base; the pair decreases by one, or down to zero
    for (const uint64_t base : bases)
        for (size_t n = 1; n <= 9; n++)
            for (size_t at = 0; at < n; at++)
                for (int to_zero = 0; to_zero < 2; to_zero++) {
                    std::vector<uint64_t> offsets(n + 1);
                    for (size_t i = 0; i <= n; i++) offsets[i] = base + 1 + 100 * i;
                    offsets[at + 1] = to_zero ? 0 : offsets[at] - 1;
                    const size_t before = refused;
                    check_rebase(offsets, refused);
                    CHECK(refused == before + 1);
                    cases++;
                }
    CHECK(refused < cases);
    printf("offsets: %zu arrays, %zu refused, the property holds\n", cases, refused);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "plan") return run_plan();
    if (argc == 4 && std::string(argv[1]) == "program") return run_program(argv[2], argv[3]);
    if (argc == 4 && std::string(argv[1]) == "buckets") return run_buckets((uint32_t)atoi(argv[2]), atoi(argv[3]));
    if (argc == 4 && std::string(argv[1]) == "passes") return run_passes((uint32_t)atoi(argv[2]), atoi(argv[3]));
    if (argc == 4 && std::string(argv[1]) == "offsets") return run_offsets((uint32_t)atoi(argv[2]), atoi(argv[3]));
    fprintf(stderr, "usage: host_logic_asan program <hints> <out> | buckets <seed> <rounds> | passes <seed> <rounds> | offsets <seed> <rounds> | plan\n");
    return 2;
}
