// verify_api.inc — host launcher of the verify pipeline (included by rsv_hip.hip).  The decisions that touch no device
// (shape buckets, workspace groups) live in host_logic.hpp, where a sanitizer can reach them.
//
// Launch plan for one batch (M = main stream, S = side stream):
//   1. M: k_parse over the whole batch, then ONE 32-byte read-back of the batch summary (max queries / log size /
//      FRI layers, and whether all proofs share one shape) over S while M goes on with
//   2. M: k_transcript (needs nothing from the host);
//   3. shape buckets: a uniform batch is one bucket in natural order; a mixed batch is bucketed by n_queries on
//      the host (8 bytes per proof read back, one index list uploaded) so every launch uses exactly
//      G = n_queries lanes per proof;  S: k_row_hash underneath the transcript, then k_qconst;
//   4. per group of buckets (a group = what fits the workspace budget, normally the whole batch):
//      M: k_plan -> k_trace_merkle;  S: k_query -> k_pair_merkle (single-group batches: the FRI trees run next to the
//      trace trees; with several groups k_pair_merkle follows k_trace_merkle on M, the groups share the workspace);
//   5. k_oods, which only feeds k_finalize: on M behind the trace trees (single group) or last on S; with per-proof public
//      inputs (rsv_verify_batch_inputs_dev) k_pi_sum right in front of it on the same stream;
//   6. M, behind everything on S: k_finalize over the whole batch — verdicts, the canonicity fallback for proofs whose
//      witness lists had the wrong length (layout.hpp), optionally the accept bitmap.
// No hipMalloc happens after the two workspaces have grown to the batch shape once.

namespace {

constexpr int kBlock = 256;
// Row form of the tree kernels (k_merkle.hpp): 512 threads = 32 virtual lanes per workgroup (two waves per SIMD: 256 registers); chosen while the FRI-tree
// launch holds at most this many paths (proofs x queries x trees).
constexpr int kRowTreeBlock = 512;
constexpr uint64_t kRowTreeLanes = 256ull * 16 * 9;
constexpr uint64_t kRowQueryLanes = 256ull * 16;  // k_query's row form: up to this many queries (proofs x queries) in the launch

using rsv::host::Carve;

struct StageClock {
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    hipEvent_t next() {
        if (used == pool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            pool.push_back(e);
        }
        return pool[used++];
    }
};

const char* const kStageNames[] = {"parse", "transcript", "oods", "plan", "query", "trace_merkle", "pair_merkle", "finalize", "cap_top(span)", "row_hash(overlapped)", "qconst(overlapped)"};
constexpr int kNumStages = 11;

struct VerifyState {
    StageClock clock;
    // (stage index, begin event, end event)
    struct Span { int stage; hipEvent_t b, e; };
    std::vector<Span> spans;
    std::vector<uint32_t> h_shape, h_ids;  // host staging for mixed-shape batches
    std::vector<uint32_t> h_class;
};

VerifyState* state_of(rsv_ctx* c) {
    if (!c->vs) c->vs = new VerifyState();
    return c->vs;
}
void destroy_verify_state(VerifyState* v) {
    for (auto e : v->clock.pool) (void)hipEventDestroy(e);
    delete v;
}

// every stream of the context is idle: what ensure_buf waits for before it frees, and before it fills (RSV_OPT_WS_FILL).
// The aux stream is joined into the main one by every call that uses it (ev_fork), except on an error exit taken between
// the parser's launch and that join: a buffer freed behind such an exit could still be the parser's target.
int ws_idle(rsv_ctx* c) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->side));
    HIP_TRY(hipStreamSynchronize(c->aux));
    return RSV_OK;
}

// RSV_OPT_WS_FILL (diagnostic): every byte of `bytes` at `p` holds the fill byte before the call goes on.  Host-synchronous
// on purpose: the streams are idle in front of the fill and the fill is over behind it, whatever stream touches `p` next.
int ws_fill(rsv_ctx* c, void* p, size_t bytes) {
    if (!p || !bytes) return RSV_OK;
    const int rc = ws_idle(c);
    if (rc != RSV_OK) return rc;
    HIP_TRY(hipMemsetAsync(p, c->opt.ws_fill - 1, bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSV_OK;
}

int ensure_buf(rsv_ctx* c, void** buf, size_t* cap, size_t bytes) {
    if (*cap < bytes) {
        const int rc = ws_idle(c);
        if (rc != RSV_OK) return rc;
        if (*buf) (void)hipFree(*buf);
        *buf = nullptr;
        *cap = 0;
        size_t want = bytes + (bytes >> 3) + 4096;
        HIP_TRY(hipMalloc(buf, want));
        *cap = want;
    }
    if (c->opt.ws_fill) return ws_fill(c, *buf, *cap);  // the whole capacity, slack included, grown or not
    return RSV_OK;
}

size_t ws_budget(const rsv_ctx* c) { return (size_t)c->opt.ws_budget_mb << 20; }

}  // namespace

namespace {
// optional output of the per-query trace-tree paths (rsv_trace_paths_dev)
struct PathsOut {
    uint32_t* d_sib;   // trace trees (nullptr: not requested)
    uint32_t* d_pos;
    uint32_t n_queries, max_log;
    uint32_t* d_pair_sib;   // FRI trees (nullptr: not requested)
    uint32_t* d_pair_cols;
    uint32_t n_inner;
    uint32_t* d_transcript;  // [n][RSV_TRANSCRIPT_WORDS] (nullptr: not requested)
    uint32_t* d_folded;      // [n][3][nq][4] first-layer folds (nullptr: not requested; needs d_pair_sib)
    uint32_t* d_cols;        // trace trees: [n][4][nq][64] column values per path (nullptr: not requested)
    uint32_t* d_qv;          // [n][nq][4 * (8 + n_inner)] per-query quotient / fold values (nullptr: not requested)
    FlowArgs flow;           // PoseidonFlow records (rec == nullptr: not requested); any mix of shapes
    uint32_t* d_bitmap;      // accept bitmap of the batch, written by k_finalize (nullptr: not requested)
    uint64_t* d_count;       // its popcount (may be null)
    bool paths() const { return d_sib || d_pair_sib || d_qv || d_cols || d_pair_cols; }  // outputs indexed by ONE declared shape
};
static_assert(TR_WORDS == RSV_TRANSCRIPT_WORDS, "include/rsv.h");
}  // namespace

extern "C" int rsv_cfg_check(const rsv_pcs_config* cfg) {
    if (!cfg) return RSV_E_NULL;
    static_assert(MAXQ == RSV_MAX_QUERIES && MAX_LOG == RSV_MAX_LOG_SIZE && MAX_INNER == RSV_MAX_FRI_INNER, "include/rsv.h");
    if (cfg->n_queries < 1 || cfg->n_queries > RSV_MAX_QUERIES || cfg->log_blowup_factor < 1 || cfg->log_blowup_factor > RSV_MAX_LOG_BLOWUP ||
        cfg->log_last_layer_degree_bound > RSV_MAX_LOG_LAST_LAYER || cfg->pow_bits > RSV_MAX_POW_BITS)
        return RSV_E_SIZE;
    return RSV_OK;
}

// what every entry point checks of its rsv_cfg_set before anything else
static int check_cfg_set(const rsv_cfg_set* cfg) {
    if (!cfg || !cfg->cfgs) return RSV_E_NULL;
    if (cfg->n_cfgs < 1 || cfg->n_cfgs > (uint32_t)RSV_MAX_CFGS) return RSV_E_SIZE;
    for (uint32_t k = 0; k < cfg->n_cfgs; k++)  // a configuration beyond the library's shape limits is misuse, not n parse rejects
        if (rsv_cfg_check(&cfg->cfgs[k]) != RSV_OK) return RSV_E_SIZE;
    return RSV_OK;
}

// rsv_cfg_set -> the by-value kernel argument (cfg_of stays whatever pointer the caller gave: device memory here)
static int make_cfg_set(const rsv_cfg_set* cfg, CfgSet* out) {
    {
        const int rc0 = check_cfg_set(cfg);
        if (rc0 != RSV_OK) return rc0;
    }
    static_assert(MAX_CFGS == RSV_MAX_CFGS, "include/rsv.h");
    memset(out, 0, sizeof(*out));
    out->n = cfg->n_cfgs;
    for (uint32_t k = 0; k < cfg->n_cfgs; k++) {
        out->c[k][0] = cfg->cfgs[k].pow_bits; out->c[k][1] = cfg->cfgs[k].log_blowup_factor;
        out->c[k][2] = cfg->cfgs[k].log_last_layer_degree_bound; out->c[k][3] = cfg->cfgs[k].n_queries;
    }
    out->cfg_of = cfg->cfg_of;
    return RSV_OK;
}

// the OODS evaluation has a lane form and (later) a row form; both entry points launch through here
// small batches: one proof per 16-lane row (latency form); large ones: one proof per lane (throughput form).
// RSV_OPT_OODS_FORM overrides (tests).  The row form is a latency form: it pays while the kernel is on the step's chain
// of dependent kernels; since it runs behind the trace trees beside k_pair_merkle (and costs three times the issue slots
// per proof) the lane form wins from 8 192 proofs on (4 096: 2.82 vs 2.97 ms; 8 192: 5.43 vs 5.38; 16 384: 10.31 vs
// 10.14; 24 576: 15.09 vs 14.67).
static bool oods_row_form(const Options& o, size_t n) { return o.oods_form ? o.oods_form == 1 : n <= 6144; }
static void launch_oods_probe(const uint32_t* d_prefix, uint32_t prefix_words, const uint32_t* d_params, uint32_t* d_out, uint32_t n) {
    if (oods_row_form(default_options(), n))
        hipLaunchKernelGGL(k_oods_row_probe, dim3(grid_for((size_t)n * 16, 256)), dim3(256), 0, 0, d_prefix, prefix_words, d_params, d_out, n);
    else
        hipLaunchKernelGGL(k_oods_probe, dim3(grid_for(n, 64)), dim3(64), 0, 0, d_prefix, prefix_words, d_params, d_out, n);
}

static int verify_impl(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                       const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, const rsv_public_input* d_own_pi,
                       uint8_t* d_accept, uint8_t* d_reason, const PathsOut* po) {
    // d_own_pi: nullptr — `pi` is the batch's one table, in host memory; else [n][n_pi] records in HBM, every proof its own
    // (`pi` is unused): k_pi_sum sums them per proof and the OODS kernel reads that sum (k_pi_sum.hpp)
    if (!c) return RSV_E_NULL;
    CfgSet co;
    {
        int rc0 = make_cfg_set(cfg, &co);  // required even for an empty batch: a caller that forgot it learns at once
        if (rc0 != RSV_OK) return rc0;
    }
    if (n == 0) return RSV_OK;
    if (!d_blob || !d_offsets || !d_accept) return RSV_E_NULL;
    const bool own = d_own_pi != nullptr;
    if (n_pi && !pi && !own) return RSV_E_NULL;
    if (n > (1u << 26) || n_pi > 4096) return RSV_E_SIZE;
    if (own && (uint64_t)n * n_pi > RSV_MAX_INPUT_RECORDS) return RSV_E_SIZE;
    if (((uintptr_t)d_blob & 3) || ((uintptr_t)d_offsets & 7) || ((uintptr_t)d_own_pi & 3)) return RSV_E_SIZE;
    for (size_t i = 0; i < n_pi && !own; i++)
        for (int k = 0; k < 4; k++)
            if (pi[i].value[k] >= RSV_M31_P) return RSV_E_RANGE;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const Options opt = c->opt;
    VerifyState* vs = state_of(c);
    vs->clock.used = 0;
    vs->spans.clear();
    // Stage clock: opt-in (RSV_OPT_STAGE_TIMES).  Two event records around a stage cost ~8 us of queue time EACH STAGE
    // (tools/chain_lab.hip: 5.3 us per dependent empty launch, 13.3 with the two records) — on a small batch's chain of
    // seven stages that was 4 % of the call, paid by every caller for a diagnostic only bench.py reads.
    const bool timing = opt.stage_times == 1;
    auto begin_on = [&](int stage, hipStream_t on) {
        if (!timing) return;
        hipEvent_t b = vs->clock.next();
        if (b) (void)hipEventRecord(b, on);
        vs->spans.push_back({stage, b, nullptr});
    };
    auto end_on = [&](hipStream_t on) {
        if (!timing) return;
        hipEvent_t e = vs->clock.next();
        if (e) (void)hipEventRecord(e, on);
        for (size_t i = vs->spans.size(); i-- > 0;)  // the span opened last and not yet closed
            if (!vs->spans[i].e) { vs->spans[i].e = e; break; }
    };
    auto begin = [&](int stage) { begin_on(stage, st); };
    auto end = [&]() { end_on(st); };

    const uint32_t N = (uint32_t)n;
    // public inputs
    if (c->d_pi_cap < n_pi + 1) {
        if (c->d_pi) (void)hipFree(c->d_pi);
        c->d_pi = nullptr;
        c->d_pi_cap = 0;
        HIP_TRY(hipMalloc((void**)&c->d_pi, sizeof(rsv_public_input) * (n_pi + 16)));
        c->d_pi_cap = n_pi + 16;
    }
    if (opt.ws_fill) {  // in front of the copy (the shared table) or of nothing (per-proof inputs never read it)
        const int rcf = ws_fill(c, c->d_pi, sizeof(rsv_public_input) * c->d_pi_cap);
        if (rcf != RSV_OK) return rcf;
    }
    if (n_pi && !own) HIP_TRY(hipMemcpyAsync(c->d_pi, pi, sizeof(rsv_public_input) * n_pi, hipMemcpyHostToDevice, st));
    // rsv_hints_out::d_query_values: "absent groups, and the rows of a proof the parser rejected, are zero" holds for the caller's buffer as it is
    if (po && po->d_count) HIP_TRY(hipMemsetAsync(po->d_count, 0, 8, st));
    if (po && po->d_qv)
        HIP_TRY(hipMemsetAsync(po->d_qv, 0, (size_t)N * po->n_queries * 4 * (8 + (size_t)po->n_inner) * sizeof(uint32_t), st));
    static_assert(sizeof(rsv_public_input) == sizeof(PubInput), "layout");

    // whole-batch records (their own allocation: growing the per-query workspace never moves them)
    Carve fixed{nullptr};
    fixed.take<uint32_t>(64);
    fixed.take<ProofMeta>(N);
    fixed.take<ProofCtx>(N);
    fixed.take<uint32_t>(2 * (size_t)N);
    fixed.take<uint32_t>(N);
    fixed.take<ClassTable>(1);
    fixed.take<uint8_t>(N);
    fixed.take<uint32_t>(own ? 4 * (size_t)N : 0);
    int rc = ensure_buf(c, &c->ws_fixed, &c->ws_fixed_bytes, fixed.off);
    if (rc != RSV_OK) return rc;
    Carve cv{static_cast<char*>(c->ws_fixed)};
    uint32_t* summary = cv.take<uint32_t>(64);
    ProofMeta* metas = cv.take<ProofMeta>(N);
    c->last_metas = metas;
    ProofCtx* ctxs = cv.take<ProofCtx>(N);
    uint32_t* d_shape = cv.take<uint32_t>(2 * (size_t)N);
    uint32_t* d_ids = cv.take<uint32_t>(N);
    ClassTable* d_classes = cv.take<ClassTable>(1);
    uint8_t* d_cls = cv.take<uint8_t>(N);
    uint32_t* d_pi_sum = cv.take<uint32_t>(own ? 4 * (size_t)N : 0);  // k_pi_sum -> k_oods<PiOwn>

    // small batches: one proof per 16-lane DPP row (latency form of the transcript); large ones: one proof per lane
    // (throughput form).  RSV_OPT_TRANSCRIPT_FORM overrides (tests).
    bool row = N <= 24576;  // measured crossover on MI355X: 16 384 proofs 1.41 M/s (row) vs 1.26 M/s (lane), 32 768: 1.32 vs 1.36
    if (opt.transcript_form) row = opt.transcript_form == 1;
    const bool flow = po && po->flow.rec;
    const FlowArgs fargs = flow ? po->flow : FlowArgs{nullptr, nullptr, nullptr, 0};
    if (flow) {
        if (fargs.count) HIP_TRY(hipMemsetAsync(fargs.count, 0, sizeof(uint32_t) * (size_t)N, st));
    }
    // Up to one wave per SIMD (4 096 proofs) the row form runs as two launches: the front half needs nothing from the
    // parser and starts next to it on the aux stream (k_transcript.hpp): 1 024 proofs 1.67 -> 1.63 ms, 4 096 2.89 -> 2.82;
    // at 8 192 it is a wash and beyond that the two halves and the parser get in each other's way (12 288: +12 %).
    // RSV_OPT_TRANSCRIPT_SPLIT overrides (tests).  The lane form (large batches) always runs as one launch (split the same
    // way, it measured 35.46 vs 35.20 ms at 65 536 proofs: inside run-to-run noise), and so does a pass that writes the flow.
    const bool split = row && !flow && (opt.transcript_split ? opt.transcript_split == 2 : N <= 4096);
    // Split: the PARSER goes to the aux stream and the front half stays on the main stream, in front of the back half — the
    // parser (0.04-0.1 ms) is long over when the front half (0.16-0.19 ms) ends, so the back half's wait for it is a wait
    // for an event signalled long ago, and front -> back is a boundary inside one stream (~5 us) instead of a fresh
    // cross-stream wait (15 us; until the end of round 4 the front half was the one on the aux stream).
    hipStream_t parse_on = split ? c->aux : st;
    if (split) {
        HIP_TRY(hipEventRecord(c->ev_begin, st));  // behind whatever produced the blob, the offsets and the inputs
        HIP_TRY(hipStreamWaitEvent(c->aux, c->ev_begin, 0));
    }
    begin_on(0, parse_on);
    HIP_TRY(hipMemsetAsync(summary, 0, 256, parse_on));
    hipLaunchKernelGGL(k_parse, dim3(grid_for(N, 64)), dim3(64), 0, parse_on, d_blob, d_offsets, N, co, metas, ctxs, summary, d_shape);
    end_on(parse_on);
    HIP_TRY(hipGetLastError());
    // The transcript needs nothing from the host: it is enqueued right behind the parser, and the parse summary
    // (and, for mixed batches, the shape words) travel back through the side stream while it runs.
    HIP_TRY(hipEventRecord(c->ev_fork, parse_on));
    if (split) {
        hipLaunchKernelGGL(k_transcript_row<1>, dim3(grid_for((size_t)N * 16, 256)), dim3(256), 0, st, d_blob, d_offsets, N, metas, ctxs, fargs);
        HIP_TRY(hipStreamWaitEvent(st, c->ev_fork, 0));  // everything behind this on the main stream may read the parser's tables
    }
    begin(1);
    if (split)
        hipLaunchKernelGGL(k_transcript_row<2>, dim3(grid_for((size_t)N * 16, 256)), dim3(256), 0, st, d_blob, d_offsets, N, metas, ctxs, fargs);
    else if (row && flow)
        hipLaunchKernelGGL((k_transcript_row<0, true>), dim3(grid_for((size_t)N * 16, 256)), dim3(256), 0, st, d_blob, d_offsets, N, metas, ctxs, fargs);
    else if (row)
        hipLaunchKernelGGL(k_transcript_row<0>, dim3(grid_for((size_t)N * 16, 256)), dim3(256), 0, st, d_blob, d_offsets, N, metas, ctxs, fargs);
    else if (flow)
        hipLaunchKernelGGL(k_transcript<true>, dim3(grid_for(N, 64)), dim3(64), 0, st, d_blob, d_offsets, N, metas, ctxs, fargs);
    else if (N <= 49152)  // (one wave per SIMD: the unpaced channel, k_transcript.hpp)
        hipLaunchKernelGGL((k_transcript<false, false>), dim3(grid_for(N, 64)), dim3(64), 0, st, d_blob, d_offsets, N, metas, ctxs, fargs);
    else
        hipLaunchKernelGGL((k_transcript<false, true>), dim3(grid_for(N, 64)), dim3(64), 0, st, d_blob, d_offsets, N, metas, ctxs, fargs);
    end();
    HIP_TRY(hipEventRecord(c->ev_tr, st));
    HIP_TRY(hipGetLastError());
    uint32_t sum[8] = {0};
    HIP_TRY(hipStreamWaitEvent(c->side, c->ev_fork, 0));
    // A batch under ONE configuration is one launch geometry of known size (n_queries is the configuration's, every
    // proof either carries it or is rejected by the parser): nothing has to come back to the host.  The slot order by
    // shape class is made on the device (k_parse.hpp) and the tables are sized for the largest trees the parser lets
    // through, so the call enqueues everything and returns: no host synchronisation anywhere in it.  Batches under
    // several configurations (several n_queries buckets whose sizes only the device knows) and calls with per-query path
    // outputs (one declared shape, checked on the host) keep the round trip of rounds 1-2 below.
    const bool device_order = co.n == 1 && !co.cfg_of && !(po && po->paths()) && opt.device_order != 2 && co.c[0][3] >= 1 &&
                              co.c[0][3] <= (uint32_t)MAXQ && co.c[0][1] >= 1 && co.c[0][1] <= 16 && co.c[0][2] <= 16;
    if (device_order) {
        HIP_TRY(hipMemsetAsync(d_classes, 0, sizeof(ClassTable), c->side));
        hipLaunchKernelGGL(k_classify, dim3(grid_for(N, CLASSIFY_PER_BLOCK)), dim3(256), 0, c->side, N, d_shape, d_classes, d_cls);
        hipLaunchKernelGGL(k_class_offsets, dim3(1), dim3(64), 0, c->side, d_classes);
        hipLaunchKernelGGL(k_scatter_ids, dim3(grid_for(N, 256)), dim3(256), 0, c->side, N, d_cls, d_classes, d_ids);
        sum[0] = 1;
    } else {
        HIP_TRY(hipMemcpyAsync(sum, summary, 32, hipMemcpyDeviceToHost, c->side));
        HIP_TRY(hipStreamSynchronize(c->side));
    }

    // A batch whose FRI-tree launch puts fewer than about two and a half waves on a SIMD (at most 1 024 proofs of 16 queries
    // and nine trees; measured: one proof 1.31 -> 1.21 ms, 512 proofs 1.43 -> 1.34, 768: 1.45 -> 1.35, 1 024: 1.467 -> 1.457,
    // 2 048: 1.906 -> 1.945, slower) runs the
    // tree kernels on the unpaced permutation instances.  An estimate from the configuration (the batch's real depth is on
    // the device only): proofs x queries x (FRI trees of the common depth M = 22).
    // Up to 256 proofs of 16 queries the trees go one step further, to the ROW form on virtual lanes (k_merkle.hpp): 16 threads per
    // path, every permutation shared by a DPP row.  RSV_OPT_TREE_PACE overrides (1 paced, 2 unpaced, 3 row).
    int tree_form = 1;  // the PACE / FORM template argument of the tree kernels: 1 paced, 0 unpaced, 2 row
    {
        const uint32_t nq_est = co.c[0][3] < 4 ? 4u : co.c[0][3], fold_est = co.c[0][1] + co.c[0][2];
        const uint64_t lanes = (uint64_t)N * nq_est * (22u > fold_est ? 22u - fold_est : 1u);
        if (opt.tree_pace) tree_form = opt.tree_pace == 1 ? 1 : (opt.tree_pace == 2 ? 0 : 2);
        else if (co.n == 1 && lanes <= (uint64_t)kRowTreeLanes) tree_form = 2;
        else if (co.n == 1 && lanes <= 1024ull * 16 * 9) tree_form = 0;
        if (flow && tree_form == 0) tree_form = 1;  // (the FLOW instantiations: paced lane form and row form)
    }
    const bool small_trees = tree_form != 1;  // (the row hashes: lane forms only; they run underneath the transcript)
    if (sum[0] > 0) {
        // shape buckets: one launch geometry per distinct n_queries (host_logic.hpp)
        using rsv::host::Bucket;
        std::vector<Bucket> buckets;
        const bool uniform = !device_order && sum[4] == ~sum[5] && sum[6] == ~sum[7];
        if (device_order) {
            // every slot of the batch (rejected proofs have no live lane), the deepest trees the parser admits
            const uint32_t b = co.c[0][1], last = co.c[0][2];
            const uint32_t inner_bound = (uint32_t)MAX_LOG - 1u - (last + b);
            buckets.push_back({co.c[0][3], (uint32_t)MAX_LOG, inner_bound > (uint32_t)MAX_INNER ? (uint32_t)MAX_INNER : inner_bound, last + b + 1u, N, 0});
        } else
        if (po && po->paths() && (!uniform || (sum[4] & 0xFFu) != po->n_queries || ((sum[4] >> 8) & 0xFFu) != po->max_log || po->n_queries < 4 ||
                   ((po->d_pair_sib || po->d_pair_cols || po->d_qv) && ((sum[4] >> 16) & 0xFFu) != po->n_inner)))
            return RSV_E_SIZE;  // path emission needs one shape for the whole batch, as declared by the caller
        if (device_order) {
        } else if (uniform) {
            buckets.push_back({sum[4] & 0xFFu, (sum[4] >> 8) & 0xFFu, (sum[4] >> 16) & 0xFFu, sum[4] >> 24, N, 0});
        } else {
            // Mixed batch: 8 bytes per proof come back, the host buckets them (rsv::host::bucket_by_shape) and uploads the
            // slot -> proof list.
            std::vector<uint32_t>& shape = vs->h_shape;
            shape.resize(2 * (size_t)N);
            HIP_TRY(hipMemcpyAsync(shape.data(), d_shape, 8 * (size_t)N, hipMemcpyDeviceToHost, c->side));
            HIP_TRY(hipStreamSynchronize(c->side));
            std::vector<uint32_t>& ids = vs->h_ids;
            rsv::host::bucket_by_shape(shape.data(), N, buckets, ids, vs->h_class);
            if (!ids.empty()) HIP_TRY(hipMemcpyAsync(d_ids, ids.data(), 4 * ids.size(), hipMemcpyHostToDevice, c->side));
        }
        // the slot -> proof list was uploaded on the side stream: k_plan (main stream) waits for it
        HIP_TRY(hipEventRecord(c->ev_ids, c->side));
        HIP_TRY(hipStreamWaitEvent(st, c->ev_ids, 0));
        HIP_TRY(hipGetLastError());
        // Side stream: trace-tree column hashing (independent of the transcript), so that it fills the issue slots the
        // one-wave-per-SIMD transcript kernel leaves idle.  Row hashes are addressed by SLOT and sized per bucket
        // (count x that bucket's n_queries): one well-formed 128-query header in a batch of 16-query proofs must not
        // inflate the allocation of the whole batch.  All buckets go into ONE launch (Fused<>, at most MAX_FUSED each).
        std::vector<size_t> row_base(buckets.size());
        size_t row_words = 0;
        for (size_t bi = 0; bi < buckets.size(); bi++) {
            const uint32_t gq = buckets[bi].G < 4 ? 4u : buckets[bi].G;
            row_base[bi] = row_words;
            row_words += (size_t)buckets[bi].count * 4 * 2 * gq * 8;
        }
        rc = ensure_buf(c, &c->ws_rows, &c->ws_rows_bytes, row_words * 4);
        if (rc != RSV_OK) return rc;
        uint32_t* rowh = static_cast<uint32_t*>(c->ws_rows);
        {
            begin_on(9, c->side);
            for (size_t b0 = 0; b0 < buckets.size(); b0 += MAX_FUSED) {
                Fused<RowHashArgs> fr{};
                uint32_t blocks = 0;
                for (size_t bi = b0; bi < buckets.size() && bi < b0 + MAX_FUSED; bi++) {
                    const Bucket& b = buckets[bi];
                    const uint32_t gq = b.G < 4 ? 4u : b.G;
                    fr.first_block[fr.nb] = blocks;
                    fr.a[fr.nb++] = RowHashArgs{d_blob, d_offsets, b.count, gq, metas, rowh + row_base[bi], uniform ? nullptr : d_ids + b.first, ctxs};
                    blocks += grid_for((size_t)b.count * gq, kBlock);
                }
                fr.first_block[fr.nb] = blocks;
                // a small batch's launches leave a wave nearly alone on its SIMD: the unpaced permutation instances (poseidon2.hpp)
                if (small_trees) hipLaunchKernelGGL(k_row_hash<false>, dim3(blocks, 4), dim3(kBlock), 0, c->side, fr);
                else hipLaunchKernelGGL(k_row_hash<true>, dim3(blocks, 4), dim3(kBlock), 0, c->side, fr);
            }
            end_on(c->side);
            HIP_TRY(hipEventRecord(c->ev_join, c->side));
        }
        // query-independent quotient constants: need only the transcript (launched below, once the stream layout is known)
        // the row form of the quotient constants on four rows per proof (k_plan.hpp: qconst_row_body); RSV_OPT_QCONST_FORM = 1
        // forces the row form with ONE row per proof (what batches of 4 097 .. 24 576 proofs run), so that tests reach it
        const bool qconst4 = N <= 4096 && opt.qconst_form != 1;
        auto launch_qconst = [&](hipStream_t on) {
            begin_on(10, on);
            // small batches: one proof per 16-lane row (latency form); RSV_OPT_QCONST_FORM overrides (tests)
            const bool qrow = opt.qconst_form ? opt.qconst_form == 1 : N <= 24576;
            if (qrow)
                hipLaunchKernelGGL(k_qconst_row, dim3(grid_for((size_t)N * (qconst4 ? 64 : 16), 256)), dim3(256), 0, on, d_blob, d_offsets,
                                   N | (qconst4 ? 0x80000000u : 0u), metas, ctxs);
            else
                hipLaunchKernelGGL(k_qconst, dim3(grid_for(N, 64)), dim3(64), 0, on, d_blob, d_offsets, N, metas, ctxs);
            end_on(on);
        };

        bool oods_launched = false;
        auto launch_oods = [&](hipStream_t on) {
            begin_on(2, on);
            const PiShared shared{reinterpret_cast<const PubInput*>(c->d_pi), (uint32_t)n_pi};
            const PiOwn sums{d_pi_sum};
            // per-proof inputs: the statement sums first, on the same stream (behind the transcript, as the OODS kernel is)
            if (own)
                hipLaunchKernelGGL(k_pi_sum<true>, dim3(grid_for(N, PI_WAVES)), dim3(64 * PI_WAVES), 0, on, reinterpret_cast<const uint32_t*>(d_own_pi),
                                   N, (uint32_t)n_pi, metas, ctxs, (const uint32_t*)nullptr, d_pi_sum, (uint8_t*)nullptr);
            if (oods_row_form(opt, N)) {
                if (own) hipLaunchKernelGGL(k_oods_row<PiOwn>, dim3(grid_for((size_t)N * 16, 256)), dim3(256), 0, on, d_blob, d_offsets, N, metas, ctxs, sums);
                else hipLaunchKernelGGL(k_oods_row<PiShared>, dim3(grid_for((size_t)N * 16, 256)), dim3(256), 0, on, d_blob, d_offsets, N, metas, ctxs, shared);
            } else {
                if (own) hipLaunchKernelGGL(k_oods<PiOwn>, dim3(grid_for(N, 64)), dim3(64), 0, on, d_blob, d_offsets, N, metas, ctxs, sums);
                else hipLaunchKernelGGL(k_oods<PiShared>, dim3(grid_for(N, 64)), dim3(64), 0, on, d_blob, d_offsets, N, metas, ctxs, shared);
            }
            end_on(on);
            oods_launched = true;
        };

        // Per-query stages.  The batch is cut into GROUPS of at most MAX_FUSED (bucket, slot range) entries whose
        // workspaces fit the budget together; a group is ONE launch per stage.  A uniform batch is one entry (several
        // groups only when it exceeds the budget), a mixed batch normally one group with an entry per n_queries.
        using rsv::host::Entry;
        // The top of the cap in its own kernel (k_cap_top: one lane per tree instead of a part-filled wave per workgroup):
        // fewer permutation slots, two more launches — from 1 024 proofs on (measured: 1 024 proofs 1.663 -> 1.652 ms, 16 384: 9.98 -> 9.84, 65 536: 34.96 -> 34.37; a single proof would wait for three sequential hashes of a 17-lane launch),
        // and not while per-query paths are emitted (the cap writes the top of every path as it goes).
        const bool cap_top = !(po && (po->d_sib || po->d_pair_sib)) && (opt.cap_top ? opt.cap_top == 1 : N >= 1024);
        std::vector<std::vector<Entry>> groups;
        const rsv::host::GroupPolicy policy{ws_budget(c), (size_t)MAX_FUSED, opt.tree_cap == 2, flow, opt.flow_cap == 2, cap_top, opt.cap_mid};
        const size_t need = rsv::host::plan_groups(buckets, policy, groups);
        rc = ensure_buf(c, &c->ws, &c->ws_bytes, need);
        if (rc != RSV_OK) return rc;

        // Per group.  k_plan needs only the transcript, k_trace_merkle needs the plan and the row hashes, k_query
        // (quotients + folds) is needed only by k_pair_merkle: it runs on the side stream underneath k_trace_merkle.
        bool joined = false;
        const bool serial_plan = opt.plan_form == 2;  // one-lane-per-proof original (tests)
        for (const std::vector<Entry>& grp : groups)
            for (const Entry& en : grp)
                if (tree_form == 2 && en.G > (uint32_t)kRowTreeBlock / 16u) tree_form = flow ? 1 : 0;  // more queries than virtual lanes in a workgroup
        const uint32_t tree_lanes = tree_form == 2 ? (uint32_t)kRowTreeBlock / 16u : (uint32_t)kBlock;  // lanes of the tree kernels' indexing per workgroup
        // The FRI trees go to the SIDE stream right behind k_query (the only thing they wait for) and run next to the
        // trace trees instead of after them; the two kernels that only feed k_finalize (OODS check, canonicity scan)
        // follow the trace trees on the main stream.  A small batch leaves most of the chip idle and its step is a
        // chain of dependent kernels, so the overlap shortens it (1 024 proofs -3 %, 2 048 -4 %, 8 192 -2.4 %); a
        // large one fills the chip with either kernel and gains 0.4 % (65 536 proofs: 35.7 vs 35.9 ms).  Batches cut
        // into several groups keep the serial order: the groups share one workspace.
        bool overlap_trees = groups.size() == 1;
        if (opt.overlap_trees == 2) overlap_trees = false;
        // Stream layout of a single-group batch.  "Chain" (RSV_OPT_CRITICAL_CHAIN): every kernel the verdict waits for
        // longest sits on ONE stream, in order — transcript, quotient constants, plan, k_query, FRI trees, finalize — and
        // the side stream takes what finishes early anyway (row hashes, then — behind the plan — trace trees and the OODS
        // check).  A kernel that waits for another stream's event starts ~20 us after it (measured on MI355X: 18-28 us
        // against 5-11 us behind a kernel of its own stream); the two-stream layout of rounds 1-2 had three such waits
        // on the path of a small batch (transcript -> k_qconst, k_plan -> k_query, FRI trees -> finalize).
        const bool chain = overlap_trees && (opt.critical_chain ? opt.critical_chain == 1 : N <= 24576);  // measured: +1..4 % from 512 to 16 384 proofs, -2 % at 32 768 and beyond
        // the row-form quotient constants of a chain-layout batch ride in the plan's launch (k_plan_par<.., true>)
        // k_query on virtual lanes (k_query.hpp: 16 threads per query split its sums): RSV_OPT_QUERY_FORM, or by size
        bool query_row = chain && (opt.query_form ? opt.query_form == 1 : (uint64_t)N * (co.c[0][3] < 4 ? 4u : co.c[0][3]) <= (uint64_t)kRowQueryLanes && co.n == 1);
        for (const std::vector<Entry>& grp : groups)
            for (const Entry& en : grp)
                if (en.G > (uint32_t)kRowTreeBlock / 16u) query_row = false;
        const bool qconst_in_plan = chain && !serial_plan && (opt.qconst_form ? opt.qconst_form == 1 : N <= 24576);
        if (qconst_in_plan) {
        } else if (chain) launch_qconst(st);
        else {
            HIP_TRY(hipStreamWaitEvent(c->side, c->ev_tr, 0));
            launch_qconst(c->side);
        }
        for (const std::vector<Entry>& grp : groups) {
            Fused<PlanArgs> fp{};
            Fused<QueryArgs> fq{};
            Fused<MerkleArgs> fm{};
            CapTopIndex ix_t{}, ix_p{}, ix_mt{}, ix_mp{};
            uint32_t blocks = 0, blocks_m = 0, blocks_q = 0, max_inner = 0, top_t = 0, top_p = 0, mid_t = 0, mid_p = 0;  // blocks_m / _q: workgroups of the tree kernels / of k_query's row form
            bool any_top = false, any_mid = false;
            Carve wq{static_cast<char*>(c->ws)};
            for (const Entry& en : grp) {
                const Bucket& b = buckets[en.bi];
                PlanPtrs pl{};
                pl.hdr = wq.take<PlanHdr>(en.cn);
                pl.ent = wq.take<uint32_t>((size_t)en.cn * (b.maxM + 1) * en.G);
                pl.fl = wq.take<uint32_t>((size_t)en.cn * 2 * en.G);
                pl.G = en.G;
                pl.maxM = b.maxM;
                uint32_t* leafv = wq.take<uint32_t>((size_t)en.cn * (3 + b.maxInner) * en.G * 8);
                pl.ids = uniform ? nullptr : d_ids + b.first + en.c0;
                pl.p0 = uniform ? (uint32_t)en.c0 : 0u;
                const size_t c0 = en.c0;
                QueryArgs qa{d_blob, d_offsets, en.cn, metas, ctxs, pl, leafv, b.maxInner,
                             (po && po->d_folded) ? po->d_folded + c0 * 3 * en.G * 4 : nullptr,
                             (po && po->d_qv) ? po->d_qv + c0 * en.G * 4 * (8 + b.maxInner) : nullptr, 4 * (8 + b.maxInner)};
                MerkleArgs ma{d_blob, d_offsets, en.cn, metas, ctxs, pl, leafv, b.maxInner, en.Lc,
                              rowh + row_base[en.bi] + c0 * 4 * 2 * (size_t)en.G * 8, nullptr, nullptr, nullptr, nullptr, nullptr,
                              en.Lt, en.Lt2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
                if (en.Lt) {
                    ma.tcapn = wq.take<uint32_t>(((size_t)en.cn * 4 << en.Lt) * 8);
                    ma.tcapm = wq.take<unsigned long long>((size_t)en.cn * 4);
                    ma.pcapn = wq.take<uint32_t>(((size_t)en.cn * (1 + b.maxInner) << en.Lt) * 8);
                    ma.pcapm = wq.take<unsigned long long>((size_t)en.cn * (1 + b.maxInner));
                    any_top = true;
                }
                if (en.Lt2 != en.Lt) {  // the levels between the hand-over and k_cap_top's: k_cap_mid
                    ma.tcapn2 = wq.take<uint32_t>(((size_t)en.cn * 4 << en.Lt2) * 8);
                    ma.tcapm2 = wq.take<unsigned long long>((size_t)en.cn * 4);
                    ma.pcapn2 = wq.take<uint32_t>(((size_t)en.cn * (1 + b.maxInner) << en.Lt2) * 8);
                    ma.pcapm2 = wq.take<unsigned long long>((size_t)en.cn * (1 + b.maxInner));
                    any_mid = true;
                }
                if (po && po->d_sib) {
                    ma.path_sib = po->d_sib + c0 * 4 * en.G * b.maxM * 8;
                    ma.path_pos = po->d_pos + c0 * 4 * en.G;
                }
                if (po && po->d_cols) ma.path_cols = po->d_cols + c0 * 4 * en.G * 64;
                if (po && po->d_pair_sib) ma.pair_sib = po->d_pair_sib + c0 * (1 + b.maxInner) * en.G * b.maxM * 8;
                if (po && po->d_pair_cols) ma.pair_cols = po->d_pair_cols + c0 * (1 + b.maxInner) * en.G * 3 * 8;
                const uint32_t k = fp.nb;
                fp.first_block[k] = blocks;
                fq.first_block[k] = query_row ? blocks_q : blocks;
                fm.first_block[k] = blocks_m;
                ix_t.first_block[k] = top_t;
                ix_p.first_block[k] = top_p;
                top_t += grid_for((size_t)en.cn * 4, 256);
                top_p += grid_for((size_t)en.cn * (1 + b.maxInner), 256);
                ix_mt.first_block[k] = mid_t;
                ix_mp.first_block[k] = mid_p;
                if (en.Lt2 != en.Lt) {
                    mid_t += grid_for((size_t)en.cn * 4 << en.Lt2, 256);
                    mid_p += grid_for((size_t)en.cn * (1 + b.maxInner) << en.Lt2, 256);
                }
                fp.a[k] = PlanArgs{en.cn, pl};
                fq.a[k] = qa;
                fm.a[k] = ma;
                fp.nb = fq.nb = fm.nb = k + 1;
                const uint32_t per_block = kBlock / en.G, per_block_m = tree_lanes / en.G;
                blocks += (en.cn + per_block - 1) / per_block;
                blocks_m += (en.cn + per_block_m - 1) / per_block_m;
                if (query_row) blocks_q += (en.cn + (uint32_t)kRowTreeBlock / 16u / en.G - 1) / ((uint32_t)kRowTreeBlock / 16u / en.G);
                max_inner = std::max(max_inner, b.maxInner);
            }
            fp.first_block[fp.nb] = blocks;
            fq.first_block[fq.nb] = query_row ? blocks_q : blocks;
            fm.first_block[fm.nb] = blocks_m;
            {   // which FRI tree each grid row of k_pair_merkle hashes: dealt out over the compute units for a launch that is
                // resident all at once (host_logic.hpp), the identity otherwise (and with RSV_OPT_PAIR_ORDER = 2)
                uint32_t group_M = 0, live = 1 + max_inner;
                for (const Entry& en : grp) group_M = std::max(group_M, buckets[en.bi].maxM);
                if (device_order) {
                    // the launch is sized for MAX_LOG; what the batch really holds is on the device only.  The weights assume
                    // the common depth of the reference's proofs (M = 22): a batch of deeper or shallower trees is still dealt
                    // out better than row y = tree y, and any order is a correct one.
                    group_M = 22;
                    const uint32_t fold = co.c[0][1] + co.c[0][2];
                    live = group_M > fold ? group_M - fold : 1u;
                }
                for (uint32_t k = 0; k < 32; k++) fm.y_of[k] = (uint8_t)k;
                if (opt.pair_order != 2)
                    rsv::host::pair_layer_order(blocks_m, 1 + max_inner, live, group_M, (uint32_t)c->n_cu, (uint32_t)RSV_PAIR_WAVES, fm.y_of);
            }
            ix_t.first_block[fm.nb] = top_t;
            ix_p.first_block[fm.nb] = top_p;
            ix_mt.first_block[fm.nb] = mid_t;
            ix_mp.first_block[fm.nb] = mid_p;
            // item order of the cap kernels (k_merkle.hpp: CapTopIndex): tree-major for launches of >= 2^19 lanes
            const bool tm_t = (uint64_t)top_t * 256 >= (1u << 19), tm_p = (uint64_t)top_p * 256 >= (1u << 19);
            begin(3);
            if (serial_plan) {
                for (uint32_t k = 0; k < fp.nb; k++)
                    hipLaunchKernelGGL(k_plan, dim3(grid_for(fp.a[k].n, 64)), dim3(64), 0, st, d_blob, d_offsets, fp.a[k].n, metas, ctxs,
                                       fp.a[k].pl);
            } else {
                uint32_t pbmax = 1;
                for (uint32_t k = 0; k < fp.nb; k++) pbmax = std::max<uint32_t>(pbmax, kBlock / fp.a[k].pl.G);
                fp.lds_proofs = pbmax;
                if (qconst_in_plan)
                    hipLaunchKernelGGL((k_plan_par<kBlock, true>), dim3(blocks + grid_for((size_t)N * (qconst4 ? 64 : 16), 256)), dim3(kBlock), plan_lds_bytes(pbmax), st,
                                       d_blob, d_offsets, metas, ctxs, fp, N | (qconst4 ? 0x80000000u : 0u));
                else
                    hipLaunchKernelGGL((k_plan_par<kBlock, false>), dim3(blocks), dim3(kBlock), plan_lds_bytes(pbmax), st, d_blob, d_offsets, metas, ctxs, fp, 0u);
            }
            end();
            HIP_TRY(hipEventRecord(c->ev_plan, st));
            HIP_TRY(hipStreamWaitEvent(c->side, c->ev_plan, 0));
            const size_t pair_lds = ((po && po->d_pair_sib) || flow) ? (size_t)kBlock * 32 : 0;
            auto launch_pair = [&](hipStream_t on) {
                if (flow && tree_form == 2) hipLaunchKernelGGL((k_pair_merkle<kRowTreeBlock, true, FORM_ROW>), dim3(blocks_m, 1 + max_inner), dim3(kRowTreeBlock), pair_lds, on, fm, fargs);
                else if (flow) hipLaunchKernelGGL((k_pair_merkle<kBlock, true>), dim3(blocks_m, 1 + max_inner), dim3(kBlock), pair_lds, on, fm, fargs);
                else if (tree_form == 2) hipLaunchKernelGGL((k_pair_merkle<kRowTreeBlock, false, FORM_ROW>), dim3(blocks_m, 1 + max_inner), dim3(kRowTreeBlock), pair_lds, on, fm, fargs);
                else if (tree_form == 0) hipLaunchKernelGGL((k_pair_merkle<kBlock, false, 0>), dim3(blocks_m, 1 + max_inner), dim3(kBlock), pair_lds, on, fm, fargs);
                else hipLaunchKernelGGL((k_pair_merkle<kBlock, false, 1>), dim3(blocks_m, 1 + max_inner), dim3(kBlock), pair_lds, on, fm, fargs);
            };
            auto launch_trace = [&](hipStream_t on) {
                if (flow && tree_form == 2) hipLaunchKernelGGL((k_trace_merkle<kRowTreeBlock, true, FORM_ROW>), dim3(blocks_m, 4), dim3(kRowTreeBlock), 0, on, fm, fargs);
                else if (flow) hipLaunchKernelGGL((k_trace_merkle<kBlock, true>), dim3(blocks_m, 4), dim3(kBlock), 0, on, fm, fargs);
                else if (tree_form == 2) hipLaunchKernelGGL((k_trace_merkle<kRowTreeBlock, false, FORM_ROW>), dim3(blocks_m, 4), dim3(kRowTreeBlock), 0, on, fm, fargs);
                else if (tree_form == 0) hipLaunchKernelGGL((k_trace_merkle<kBlock, false, 0>), dim3(blocks_m, 4), dim3(kBlock), 0, on, fm, fargs);
                else hipLaunchKernelGGL((k_trace_merkle<kBlock, false, 1>), dim3(blocks_m, 4), dim3(kBlock), 0, on, fm, fargs);
            };
            // the last levels of the trees of a kernel, right behind it on its stream (stage 8)
            auto launch_top = [&](hipStream_t on, bool pair) {
                if (!any_top) return;
                begin_on(8, on);
                const bool tm = pair ? tm_p : tm_t, fast = tree_form == 0;  // (fast: a small batch's few waves: the permutation instance without wait states, as the tree kernels in front of it)
                const dim3 blk(256);
                if (any_mid && (pair ? mid_p : mid_t)) {  // buckets that hand over at the cap level: the levels down to k_cap_top's first
                    const dim3 grid(pair ? mid_p : mid_t);
                    const CapTopIndex& ixm = pair ? ix_mp : ix_mt;
                    if (fast && tm) hipLaunchKernelGGL((k_cap_mid<0, true>), grid, blk, 0, on, fm, ixm, pair ? 1u : 0u);
                    else if (fast) hipLaunchKernelGGL((k_cap_mid<0, false>), grid, blk, 0, on, fm, ixm, pair ? 1u : 0u);
                    else if (tm) hipLaunchKernelGGL((k_cap_mid<1, true>), grid, blk, 0, on, fm, ixm, pair ? 1u : 0u);
                    else hipLaunchKernelGGL((k_cap_mid<1, false>), grid, blk, 0, on, fm, ixm, pair ? 1u : 0u);
                }
                {
                    const dim3 grid(pair ? top_p : top_t);
                    const CapTopIndex& ixt = pair ? ix_p : ix_t;
                    if (fast && tm) hipLaunchKernelGGL((k_cap_top<0, true>), grid, blk, 0, on, fm, ixt, pair ? 1u : 0u);
                    else if (fast) hipLaunchKernelGGL((k_cap_top<0, false>), grid, blk, 0, on, fm, ixt, pair ? 1u : 0u);
                    else if (tm) hipLaunchKernelGGL((k_cap_top<1, true>), grid, blk, 0, on, fm, ixt, pair ? 1u : 0u);
                    else hipLaunchKernelGGL((k_cap_top<1, false>), grid, blk, 0, on, fm, ixt, pair ? 1u : 0u);
                }
                end_on(on);
            };
            if (chain) {
                // side: trace trees behind the row hashes (same stream) and the plan (event); main: k_query, FRI trees
                begin_on(5, c->side);
                launch_trace(c->side);
                end_on(c->side);
                launch_top(c->side, false);
                begin(4);
                if (query_row) hipLaunchKernelGGL((k_query<kRowTreeBlock, 4, true>), dim3(blocks_q), dim3(kRowTreeBlock), 0, st, fq);  // a row of 16 threads per query
                else hipLaunchKernelGGL((k_query<kBlock, 4>), dim3(blocks), dim3(kBlock), 0, st, fq);  // chain layout = small batch: the latency form
                end();
                begin(6);
                launch_pair(st);
                end();
                launch_top(st, true);
                HIP_TRY(hipGetLastError());
                continue;
            }
            begin_on(4, c->side);
            hipLaunchKernelGGL((k_query<kBlock, 2>), dim3(blocks), dim3(kBlock), 0, c->side, fq);
            end_on(c->side);
            HIP_TRY(hipEventRecord(c->ev_query, c->side));
            if (!joined) { HIP_TRY(hipStreamWaitEvent(st, c->ev_join, 0)); joined = true; }
            if (overlap_trees) {
                begin_on(6, c->side);
                launch_pair(c->side);
                end_on(c->side);
                launch_top(c->side, true);
            }
            begin(5);
            launch_trace(st);
            end();
            // single-group batch: the OODS check goes in front of the trace trees' last levels, which wait for the FRI
            // trees to leave them room — so it runs underneath the FRI trees, not behind them
            if (overlap_trees && !oods_launched) launch_oods(st);
            launch_top(st, false);
            if (!overlap_trees) {
                HIP_TRY(hipStreamWaitEvent(st, c->ev_query, 0));
                begin(6);
                launch_pair(st);
                end();
                launch_top(st, true);
            }
            HIP_TRY(hipGetLastError());
        }
        // The OODS composition check only raises failure flags (atomicOr) for k_finalize: behind the trace trees on the
        // main stream when the FRI trees run on the side stream (overlap_trees), else on the side stream behind k_query.
        if (!oods_launched) launch_oods((overlap_trees && !chain) ? st : c->side);
        HIP_TRY(hipEventRecord(c->ev_scan, c->side));
    }
    if (sum[0] > 0) HIP_TRY(hipStreamWaitEvent(st, c->ev_scan, 0));
    // verdicts (+ the canonicity fallback for proofs whose witness lists some stage found of the wrong length, + the
    // accept bitmap when the caller asked for it): ONE launch behind the Merkle stages
    begin(7);
    hipLaunchKernelGGL(k_finalize, dim3(grid_for(N, 256)), dim3(256), 0, st, d_blob, d_offsets, N, metas, ctxs, d_accept, d_reason, 0u,
                       po ? po->d_bitmap : nullptr, reinterpret_cast<unsigned long long*>(po ? po->d_count : nullptr));
    end();
    if (po && po->d_transcript)  // behind every stage that can find a non-canonical word: such a proof's row says RSV_R_PARSE
        hipLaunchKernelGGL(k_export_transcript, dim3(grid_for((size_t)N * TR_WORDS, 256)), dim3(256), 0, st, N, metas, ctxs,
                           po->d_transcript);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

namespace {
// host-resident rsv_cfg_set -> the same set with cfg_of staged in device memory (host-pointer entry points)
struct DevCfgSet {
    DevBuf of;
    rsv_cfg_set dev{};
    int init(const rsv_cfg_set* host, size_t n) {
        {
            const int rc0 = check_cfg_set(host);
            if (rc0 != RSV_OK) return rc0;
        }
        dev = *host;
        if (host->cfg_of && n) {
            HIP_TRY(of.alloc(n));
            HIP_TRY(hipMemcpy(of.p, host->cfg_of, n, hipMemcpyHostToDevice));
            dev.cfg_of = of.as<const uint8_t>();
        } else dev.cfg_of = nullptr;
        return RSV_OK;
    }
};
}  // namespace

extern "C" {

int rsv_verify_batch_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                         const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint8_t* d_accept,
                         uint8_t* d_reason) {
    return verify_impl(c, d_blob, d_offsets, n, cfg, pi, n_pi, nullptr, d_accept, d_reason, nullptr);
}

int rsv_trace_paths_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                        const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint32_t n_queries, uint32_t max_log, uint32_t* d_sib,
                        uint32_t* d_pos, uint8_t* d_accept, uint8_t* d_reason) {
    if (!d_sib || !d_pos) return RSV_E_NULL;
    if (n_queries < 4 || n_queries > (uint32_t)MAXQ || max_log > (uint32_t)MAX_LOG) return RSV_E_SIZE;
    PathsOut po{d_sib, d_pos, n_queries, max_log, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, FlowArgs{}, nullptr, nullptr};
    return verify_impl(c, d_blob, d_offsets, n, cfg, pi, n_pi, nullptr, d_accept, d_reason, &po);
}

int rsv_fri_paths_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, const rsv_cfg_set* cfg, const rsv_public_input* pi,
                      size_t n_pi, uint32_t n_queries, uint32_t max_log, uint32_t n_inner, uint32_t* d_sib, uint32_t* d_cols,
                      uint8_t* d_accept, uint8_t* d_reason) {
    if (!d_sib || !d_cols) return RSV_E_NULL;
    if (n_queries < 4 || n_queries > (uint32_t)MAXQ || max_log > (uint32_t)MAX_LOG || n_inner > (uint32_t)MAX_INNER) return RSV_E_SIZE;
    PathsOut po{nullptr, nullptr, n_queries, max_log, d_sib, d_cols, n_inner, nullptr, nullptr, nullptr, nullptr, FlowArgs{}, nullptr, nullptr};
    return verify_impl(c, d_blob, d_offsets, n, cfg, pi, n_pi, nullptr, d_accept, d_reason, &po);
}

int rsv_verify_batch(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                     const rsv_public_input* pi, size_t n_pi, uint8_t* accept, uint8_t* reason, int device) {
    if (n && (!blob || !offsets || !accept)) return RSV_E_NULL;
    if (n_pi && !pi) return RSV_E_NULL;
    { const int rc0 = check_cfg_set(cfg); if (rc0 != RSV_OK) return rc0; }  // (before any device work: misuse shows without a GPU)
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    DevCfgSet dcfg;
    rc = dcfg.init(cfg, n);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return RSV_E_SIZE;
    // device copies: the blob is rebased so that proof 0 starts at byte 0
    const uint64_t base = offsets[0], total = offsets[n] - base;
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
    DevBuf dblob, doffs, dacc, dreason;
    HIP_TRY(dblob.alloc(total + 16));
    HIP_TRY(doffs.alloc(8 * (n + 1)));
    HIP_TRY(dacc.alloc(n));
    HIP_TRY(dreason.alloc(n));
    HIP_TRY(hipMemcpy(dblob.p, blob + base, total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(doffs.p, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice));
    rsv_ctx* c = nullptr;
    rc = rsv_ctx_create(device, &c);
    if (rc != RSV_OK) return rc;
    rc = rsv_verify_batch_dev(c, dblob.as<const uint8_t>(), doffs.as<const uint64_t>(), n, &dcfg.dev, pi, n_pi,
                              dacc.as<uint8_t>(), dreason.as<uint8_t>());
    if (rc == RSV_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = RSV_E_DEVICE;
    if (rc == RSV_OK && hipMemcpy(accept, dacc.p, n, hipMemcpyDeviceToHost) != hipSuccess) rc = RSV_E_DEVICE;
    if (rc == RSV_OK && reason && hipMemcpy(reason, dreason.p, n, hipMemcpyDeviceToHost) != hipSuccess) rc = RSV_E_DEVICE;
    rsv_ctx_destroy(c);
    return rc;
}

}  // extern "C"

// rsv_verify_hints_dev and rsv_verify_hints_inputs_dev (d_own_pi: verify_impl)
static int verify_hints_impl(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, const rsv_cfg_set* cfg, const rsv_public_input* pi,
                             size_t n_pi, const rsv_public_input* d_own_pi, const rsv_hints_out* out, uint8_t* d_accept, uint8_t* d_reason) {
    if (!out) return RSV_E_NULL;
    if ((out->d_trace_sib == nullptr) != (out->d_trace_pos == nullptr)) return RSV_E_NULL;
    if (out->d_fri_sib && !out->d_fri_cols) return RSV_E_NULL;  // (the column values alone are fine: rsv_witness_eval_dev asks for just them)
    if (out->d_fri_folded && !out->d_fri_sib) return RSV_E_NULL;
    if ((out->d_flow == nullptr) != (out->d_flow_swap == nullptr)) return RSV_E_NULL;
    if (out->d_flow_count && !out->d_flow) return RSV_E_NULL;
    if (out->d_flow && (out->flow_stride == 0 || ((uintptr_t)out->d_flow & 15))) return RSV_E_SIZE;
    PathsOut po{out->d_trace_sib, out->d_trace_pos, out->n_queries, out->max_log, out->d_fri_sib, out->d_fri_cols, out->n_inner,
                out->d_transcript, out->d_fri_folded, out->d_trace_cols, out->d_query_values,
                FlowArgs{out->d_flow, out->d_flow_swap, out->d_flow_count, out->flow_stride}, out->d_accept_bitmap, out->d_accept_count};
    if (out->d_accept_count && !out->d_accept_bitmap) return RSV_E_NULL;
    if (po.paths() && (po.n_queries < 4 || po.n_queries > (uint32_t)MAXQ || po.max_log > (uint32_t)MAX_LOG ||
                       po.n_inner > (uint32_t)MAX_INNER))
        return RSV_E_SIZE;
    return verify_impl(c, d_blob, d_offsets, n, cfg, pi, n_pi, d_own_pi, d_accept, d_reason, &po);
}

// what the per-proof entry points check of their inputs before anything else (include/rsv.h)
static int check_own_inputs(const void* d_pi, size_t n, size_t n_pi) {
    if (n_pi && !d_pi) return RSV_E_NULL;
    if (n_pi > 4096 || (n_pi && n > RSV_MAX_INPUT_RECORDS / n_pi)) return RSV_E_SIZE;
    return RSV_OK;
}
// verify_impl keeps host vectors (buckets, groups): a std::bad_alloc out of it is RSV_E_NOMEM, as in the circuit entry points
template <class F> static int nomem_guard(F f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return RSV_E_NOMEM;
    }
}

extern "C" {

int rsv_verify_hints_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, const rsv_cfg_set* cfg, const rsv_public_input* pi,
                         size_t n_pi, const rsv_hints_out* out, uint8_t* d_accept, uint8_t* d_reason) {
    return verify_hints_impl(c, d_blob, d_offsets, n, cfg, pi, n_pi, nullptr, out, d_accept, d_reason);
}

// (no inputs at all is the shared form with an empty table: the same sum, 0, and no extra launch)
int rsv_verify_batch_inputs_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, const rsv_cfg_set* cfg,
                                const rsv_public_input* d_pi, size_t n_pi, uint8_t* d_accept, uint8_t* d_reason) {
    if (!c) return RSV_E_NULL;
    const int rc = check_own_inputs(d_pi, n, n_pi);
    if (rc != RSV_OK) return rc;
    return nomem_guard([&] { return verify_impl(c, d_blob, d_offsets, n, cfg, nullptr, n_pi, n_pi ? d_pi : nullptr, d_accept, d_reason, nullptr); });
}

int rsv_verify_hints_inputs_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, const rsv_cfg_set* cfg,
                                const rsv_public_input* d_pi, size_t n_pi, const rsv_hints_out* out, uint8_t* d_accept, uint8_t* d_reason) {
    if (!c || !out) return RSV_E_NULL;
    const int rc = check_own_inputs(d_pi, n, n_pi);
    if (rc != RSV_OK) return rc;
    return nomem_guard([&] { return verify_hints_impl(c, d_blob, d_offsets, n, cfg, nullptr, n_pi, n_pi ? d_pi : nullptr, out, d_accept, d_reason); });
}

int rsv_verify_batch_inputs(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg, const rsv_public_input* pi,
                            size_t n_pi, uint8_t* accept, uint8_t* reason, int device) {
    if (n && (!blob || !offsets || !accept)) return RSV_E_NULL;
    if (n && n_pi && !pi) return RSV_E_NULL;
    { const int rc0 = check_cfg_set(cfg); if (rc0 != RSV_OK) return rc0; }  // (before any device work: misuse shows without a GPU)
    if (n > (1u << 26)) return RSV_E_SIZE;
    { const int rc0 = check_own_inputs(pi, n, n_pi); if (rc0 != RSV_OK) return rc0; }
    for (size_t i = 0; i < n * n_pi; i++)
        for (int k = 0; k < 4; k++)
            if (pi[i].value[k] >= RSV_M31_P) return RSV_E_RANGE;
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    DevCfgSet dcfg;
    rc = dcfg.init(cfg, n);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return RSV_E_SIZE;
    const uint64_t base = offsets[0], total = offsets[n] - base;
    std::vector<uint64_t> rel;
    try {
        rel.resize(n + 1);
    } catch (const std::bad_alloc&) {
        return RSV_E_NOMEM;
    }
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
    DevBuf dblob, doffs, dacc, dreason, dpi;
    HIP_TRY(dblob.alloc(total + 16));
    HIP_TRY(doffs.alloc(8 * (n + 1)));
    HIP_TRY(dacc.alloc(n));
    HIP_TRY(dreason.alloc(n));
    HIP_TRY(dpi.alloc(sizeof(rsv_public_input) * n * n_pi + 16));
    HIP_TRY(hipMemcpy(dblob.p, blob + base, total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(doffs.p, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice));
    if (n_pi) HIP_TRY(hipMemcpy(dpi.p, pi, sizeof(rsv_public_input) * n * n_pi, hipMemcpyHostToDevice));
    rsv_ctx* c = nullptr;
    rc = rsv_ctx_create(device, &c);
    if (rc != RSV_OK) return rc;
    rc = rsv_verify_batch_inputs_dev(c, dblob.as<const uint8_t>(), doffs.as<const uint64_t>(), n, &dcfg.dev, dpi.as<const rsv_public_input>(), n_pi,
                                     dacc.as<uint8_t>(), dreason.as<uint8_t>());
    if (rc == RSV_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = RSV_E_DEVICE;
    if (rc == RSV_OK && hipMemcpy(accept, dacc.p, n, hipMemcpyDeviceToHost) != hipSuccess) rc = RSV_E_DEVICE;
    if (rc == RSV_OK && reason && hipMemcpy(reason, dreason.p, n, hipMemcpyDeviceToHost) != hipSuccess) rc = RSV_E_DEVICE;
    rsv_ctx_destroy(c);
    return rc;
}

int rsv_public_input_sum_dev(rsv_ctx* c, const rsv_public_input* d_pi, size_t n, size_t n_pi, const uint32_t* d_z_alpha, uint32_t* d_sum,
                             uint8_t* d_bad) {
    if (!c || (n && (!d_z_alpha || !d_sum))) return RSV_E_NULL;
    if (n && n_pi && !d_pi) return RSV_E_NULL;
    if (n > (1u << 26)) return RSV_E_SIZE;
    const int rc = check_own_inputs(d_pi, n, n_pi);
    if (rc != RSV_OK) return rc;
    if (((uintptr_t)d_pi & 3) || ((uintptr_t)d_z_alpha & 3) || ((uintptr_t)d_sum & 3)) return RSV_E_SIZE;
    if (n == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_pi_sum<false>, dim3(grid_for(n, PI_WAVES)), dim3(64 * PI_WAVES), 0, c->stream, reinterpret_cast<const uint32_t*>(d_pi),
                       (uint32_t)n, (uint32_t)n_pi, (const ProofMeta*)nullptr, (ProofCtx*)nullptr, d_z_alpha, d_sum, d_bad);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

// The statement digest alone (k_statement.hpp).  The crossover between its two forms, measured (profiles/HISTORY.md,
// "Statement digests"): the row form is ahead up to 24 576 groups with 8 words and with 1 024, the lane form from 32 768 and
// 49 152 on — the lane form's 1 024 waves of 65 536 groups are one per SIMD, and a group's chain of permutations is four
// times as long in it.
constexpr size_t kStatementRowMax = 24576;
// The one place that chooses the form.  flow / flow_swap (both or neither): the records of the hash, for the evaluation of a
// hashed witness program (witness_api.inc), which calls this ahead of its witness kernels.
static void statement_digest_launch(rsv_ctx* c, const rsv_public_input* d_pi, size_t n_groups, uint32_t T, rsv_public_input* d_stmt, uint8_t* d_bad,
                                    uint4* flow, uint8_t* flow_swap) {
    const size_t row_max = c->opt.statement_row_max ? (size_t)c->opt.statement_row_max - 1 : kStatementRowMax;
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(d_pi);
    uint32_t* stmt = reinterpret_cast<uint32_t*>(d_stmt);
    const bool row = n_groups <= row_max;
    const dim3 grid(grid_for(n_groups, row ? 16 : 64)), block(row ? 256 : 64);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, c->stream, rec, (uint32_t)n_groups, T, stmt, d_bad, flow, flow_swap); };
    if (flow) row ? launch(k_statement_digest<FORM_ROW, true>) : launch(k_statement_digest<0, true>);
    else row ? launch(k_statement_digest<FORM_ROW, false>) : launch(k_statement_digest<0, false>);
}
int rsv_statement_digest_dev(rsv_ctx* c, const rsv_public_input* d_pi, size_t n_groups, size_t copies, size_t n_own, rsv_public_input* d_stmt,
                             uint8_t* d_bad) {
    if (!c || (n_groups && (!d_pi || !d_stmt))) return RSV_E_NULL;
    if (copies == 0 || copies > 64 || n_own == 0 || n_own > 4096 || n_groups > (1u << 26)) return RSV_E_SIZE;
    if (n_groups > RSV_MAX_INPUT_RECORDS / (copies * n_own)) return RSV_E_SIZE;
    if (((uintptr_t)d_pi & 3) || ((uintptr_t)d_stmt & 3)) return RSV_E_SIZE;
    if (n_groups == 0) return RSV_OK;
    HIP_TRY(hipSetDevice(c->device));
    statement_digest_launch(c, d_pi, n_groups, (uint32_t)(copies * n_own), d_stmt, d_bad, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int rsv_verify_hints(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                     const rsv_public_input* pi, size_t n_pi, const rsv_hints_out* out, uint8_t* accept, uint8_t* reason,
                     int device) {
    if (!out || (n && (!blob || !offsets || !accept))) return RSV_E_NULL;
    if (n_pi && !pi) return RSV_E_NULL;
    { const int rc0 = check_cfg_set(cfg); if (rc0 != RSV_OK) return rc0; }  // (before any device work: misuse shows without a GPU)
    if (n > (1u << 20)) return RSV_E_SIZE;
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    DevCfgSet dcfg;
    rc = dcfg.init(cfg, n);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return RSV_E_SIZE;
    const uint64_t base = offsets[0], total = offsets[n] - base;
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
    // the same struct, device side: one allocation per requested output
    const size_t nq = out->n_queries, M = out->max_log, nt = 1 + (size_t)out->n_inner;
    struct Out { uint32_t* host; uint32_t* rsv_hints_out::*field; size_t words; DevBuf buf; };
    Out outs[] = {{out->d_transcript, &rsv_hints_out::d_transcript, n * (size_t)RSV_TRANSCRIPT_WORDS, {}},
                  {out->d_trace_sib, &rsv_hints_out::d_trace_sib, n * 4 * nq * M * 8, {}},
                  {out->d_trace_pos, &rsv_hints_out::d_trace_pos, n * 4 * nq, {}},
                  {out->d_trace_cols, &rsv_hints_out::d_trace_cols, n * 4 * nq * 64, {}},
                  {out->d_fri_sib, &rsv_hints_out::d_fri_sib, n * nt * nq * M * 8, {}},
                  {out->d_fri_cols, &rsv_hints_out::d_fri_cols, n * nt * nq * 3 * 8, {}},
                  {out->d_fri_folded, &rsv_hints_out::d_fri_folded, n * 3 * nq * 4, {}},
                  {out->d_query_values, &rsv_hints_out::d_query_values, n * nq * 4 * (8 + (size_t)out->n_inner), {}},
                  {out->d_flow, &rsv_hints_out::d_flow, n * (size_t)out->flow_stride * FLOW_WORDS, {}},
                  {out->d_flow_count, &rsv_hints_out::d_flow_count, n, {}},
                  {out->d_accept_bitmap, &rsv_hints_out::d_accept_bitmap, (n + 31) / 32, {}}};
    rsv_hints_out dev = *out;
    DevBuf dcount;  // the u64 output
    if (out->d_accept_count) {
        HIP_TRY(dcount.alloc(8));
        dev.d_accept_count = dcount.as<uint64_t>();
    }
    DevBuf dswap;  // the one byte-typed output
    if (out->d_flow_swap) {
        if (out->flow_stride == 0) return RSV_E_SIZE;
        HIP_TRY(dswap.alloc(n * (size_t)out->flow_stride));
        HIP_TRY(hipMemset(dswap.p, 0, n * (size_t)out->flow_stride));
        dev.d_flow_swap = dswap.as<uint8_t>();
    }
    for (Out& o : outs) {
        if (!o.host) continue;
        if (o.words == 0) return RSV_E_SIZE;  // a path output without a declared shape
        HIP_TRY(o.buf.alloc(4 * o.words));
        HIP_TRY(hipMemset(o.buf.p, 0, 4 * o.words));
        dev.*(o.field) = o.buf.as<uint32_t>();
    }
    DevBuf dblob, doffs, dacc, dreason;
    HIP_TRY(dblob.alloc(total + 16));
    HIP_TRY(doffs.alloc(8 * (n + 1)));
    HIP_TRY(dacc.alloc(n));
    HIP_TRY(dreason.alloc(n));
    HIP_TRY(hipMemcpy(dblob.p, blob + base, total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(doffs.p, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice));
    rsv_ctx* c = nullptr;
    rc = rsv_ctx_create(device, &c);
    if (rc != RSV_OK) return rc;
    rc = rsv_verify_hints_dev(c, dblob.as<const uint8_t>(), doffs.as<const uint64_t>(), n, &dcfg.dev, pi, n_pi, &dev, dacc.as<uint8_t>(),
                              dreason.as<uint8_t>());
    if (rc == RSV_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = RSV_E_DEVICE;
    for (Out& o : outs)
        if (rc == RSV_OK && o.host && hipMemcpy(o.host, o.buf.p, 4 * o.words, hipMemcpyDeviceToHost) != hipSuccess) rc = RSV_E_DEVICE;
    if (rc == RSV_OK && out->d_accept_count && hipMemcpy(out->d_accept_count, dcount.p, 8, hipMemcpyDeviceToHost) != hipSuccess) rc = RSV_E_DEVICE;
    if (rc == RSV_OK && out->d_flow_swap &&
        hipMemcpy(out->d_flow_swap, dswap.p, n * (size_t)out->flow_stride, hipMemcpyDeviceToHost) != hipSuccess) rc = RSV_E_DEVICE;
    if (rc == RSV_OK && hipMemcpy(accept, dacc.p, n, hipMemcpyDeviceToHost) != hipSuccess) rc = RSV_E_DEVICE;
    if (rc == RSV_OK && reason && hipMemcpy(reason, dreason.p, n, hipMemcpyDeviceToHost) != hipSuccess) rc = RSV_E_DEVICE;
    rsv_ctx_destroy(c);
    return rc;
}

// PoseidonFlow: records of one proof of this shape (pure host arithmetic, the same functions the kernels index with)
int rsv_poseidon_flow_count(uint32_t log_size_plonk, uint32_t log_size_poseidon, const rsv_pcs_config* cfg, uint32_t* count) {
    if (!cfg || !count) return RSV_E_NULL;
    const uint32_t b = cfg->log_blowup_factor, last = cfg->log_last_layer_degree_bound, nq = cfg->n_queries;
    if (log_size_plonk < 1 || log_size_poseidon < 1 || log_size_plonk > 28 || log_size_poseidon > 28 || b < 1 || b > 16 || last > 16 ||
        nq < 1 || nq > (uint32_t)MAXQ)
        return RSV_E_SIZE;
    const uint32_t A = log_size_plonk + b, B = log_size_poseidon + b, M = std::max(log_size_plonk + 1, log_size_poseidon + 2) + b;
    if (M > (uint32_t)MAX_LOG || A < last + b + 1 || B < last + b + 1) return RSV_E_SIZE;
    *count = flow_total(nq, M - 1 - (last + b), 1u << last, A, B, M);
    return RSV_OK;
}

int rsv_trace_paths(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                    const rsv_public_input* pi, size_t n_pi, uint32_t n_queries, uint32_t max_log, uint32_t* sib, uint32_t* pos, uint8_t* accept, uint8_t* reason,
                    int device) {
    if (n && (!sib || !pos)) return RSV_E_NULL;
    rsv_hints_out ho{};
    ho.n_queries = n_queries; ho.max_log = max_log;
    ho.d_trace_sib = sib; ho.d_trace_pos = pos;
    return rsv_verify_hints(blob, offsets, n, cfg, pi, n_pi, &ho, accept, reason, device);
}

int rsv_fri_paths(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                  const rsv_public_input* pi, size_t n_pi, uint32_t n_queries, uint32_t max_log, uint32_t n_inner, uint32_t* sib, uint32_t* cols, uint8_t* accept,
                  uint8_t* reason, int device) {
    if (n && (!sib || !cols)) return RSV_E_NULL;
    rsv_hints_out ho{};
    ho.n_queries = n_queries; ho.max_log = max_log; ho.n_inner = n_inner;
    ho.d_fri_sib = sib; ho.d_fri_cols = cols;
    return rsv_verify_hints(blob, offsets, n, cfg, pi, n_pi, &ho, accept, reason, device);
}

int rsv_transcript_batch(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg, uint32_t* out,
                         int device) {
    if (n && !out) return RSV_E_NULL;
    std::vector<uint8_t> accept(n ? n : 1);
    rsv_hints_out ho{};
    ho.d_transcript = out;
    return rsv_verify_hints(blob, offsets, n, cfg, nullptr, 0, &ho, accept.data(), nullptr, device);
}


// ---------------------------------------------------------------- a1 / a2 / a8 / line: arithmetic probes
int rsv_field_op(int op, const uint32_t* a4, const uint32_t* b4, uint32_t* out4, size_t n, int device) {
    if (n && (!a4 || !out4)) return RSV_E_NULL;
    if (op < 0 || op > RSV_F_QPOW) return RSV_E_SIZE;
    const bool binary = op == RSV_F_QADD || op == RSV_F_QSUB || op == RSV_F_QMUL || op == RSV_F_MMUL || op == RSV_F_CMUL || op == RSV_F_QPOW;
    if (n && binary && !b4) return RSV_E_NULL;
    if (n > ((size_t)1 << 26)) return RSV_E_SIZE;
    for (size_t i = 0; i < 4 * n; i++)
        if (a4[i] >= RSV_M31_P || (binary && op != RSV_F_QPOW && b4[i] >= RSV_M31_P)) return RSV_E_RANGE;
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    DevBuf da, db, dout;
    HIP_TRY(da.alloc(16 * n));
    HIP_TRY(dout.alloc(16 * n));
    HIP_TRY(hipMemcpy(da.p, a4, 16 * n, hipMemcpyHostToDevice));
    if (binary) {
        HIP_TRY(db.alloc(16 * n));
        HIP_TRY(hipMemcpy(db.p, b4, 16 * n, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_field_op, dim3(grid_for(n, 256)), dim3(256), 0, 0, op, da.as<const uint32_t>(),
                       binary ? db.as<const uint32_t>() : nullptr, dout.as<uint32_t>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out4, dout.p, 16 * n, hipMemcpyDeviceToHost));
    return RSV_OK;
}

int rsv_domain_points(uint32_t log_size, const uint32_t* q, uint32_t* xy, size_t n, int device) {
    if (n && (!q || !xy)) return RSV_E_NULL;
    if (log_size < 1 || log_size > (uint32_t)MAX_LOG || n > ((size_t)1 << 26)) return RSV_E_SIZE;
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    DevBuf dq, dxy;
    HIP_TRY(dq.alloc(4 * n));
    HIP_TRY(dxy.alloc(8 * n));
    HIP_TRY(hipMemcpy(dq.p, q, 4 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_domain_points, dim3(grid_for(n, 256)), dim3(256), 0, 0, log_size, dq.as<const uint32_t>(),
                       dxy.as<uint32_t>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(xy, dxy.p, 8 * n, hipMemcpyDeviceToHost));
    return RSV_OK;
}

int rsv_line_eval(const uint32_t* coeffs4, uint32_t log_n, const uint32_t* x, uint32_t* out4, size_t n, int device) {
    if (!coeffs4 || (n && (!x || !out4))) return RSV_E_NULL;
    if (log_n > 16 || n > ((size_t)1 << 26)) return RSV_E_SIZE;
    const size_t nc = (size_t)1 << log_n;
    for (size_t i = 0; i < 4 * nc; i++)
        if (coeffs4[i] >= RSV_M31_P) return RSV_E_RANGE;
    for (size_t i = 0; i < n; i++)
        if (x[i] >= RSV_M31_P) return RSV_E_RANGE;
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    DevBuf dc, dx, dout;
    HIP_TRY(dc.alloc(16 * nc));
    HIP_TRY(dx.alloc(4 * n));
    HIP_TRY(dout.alloc(16 * n));
    HIP_TRY(hipMemcpy(dc.p, coeffs4, 16 * nc, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dx.p, x, 4 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_line_eval, dim3(grid_for(n, 256)), dim3(256), 0, 0, dc.as<const uint32_t>(), log_n,
                       dx.as<const uint32_t>(), dout.as<uint32_t>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out4, dout.p, 16 * n, hipMemcpyDeviceToHost));
    return RSV_OK;
}

int rsv_last_layer_check(const uint32_t* coeffs4, uint32_t log_n, const uint32_t* x, const uint32_t* folded4, uint8_t* ok,
                         size_t n, int device) {
    if (!coeffs4 || (n && (!x || !folded4 || !ok))) return RSV_E_NULL;
    if (log_n > 16 || n > ((size_t)1 << 26)) return RSV_E_SIZE;
    const size_t nc = (size_t)1 << log_n;
    for (size_t i = 0; i < 4 * nc; i++)
        if (coeffs4[i] >= RSV_M31_P) return RSV_E_RANGE;
    for (size_t i = 0; i < n; i++)
        if (x[i] >= RSV_M31_P) return RSV_E_RANGE;
    for (size_t i = 0; i < 4 * n; i++)
        if (folded4[i] >= RSV_M31_P) return RSV_E_RANGE;
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    DevBuf dc, dx, df, dok;
    HIP_TRY(dc.alloc(16 * nc));
    HIP_TRY(dx.alloc(4 * n));
    HIP_TRY(df.alloc(16 * n));
    HIP_TRY(dok.alloc(n));
    HIP_TRY(hipMemcpy(dc.p, coeffs4, 16 * nc, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dx.p, x, 4 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(df.p, folded4, 16 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_last_layer_check, dim3(grid_for(n, 256)), dim3(256), 0, 0, dc.as<const uint32_t>(), log_n,
                       dx.as<const uint32_t>(), df.as<const uint32_t>(), dok.as<uint8_t>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(ok, dok.p, n, hipMemcpyDeviceToHost));
    return RSV_OK;
}

// a10 probe: scatter the flattened samples to the word offsets the kernels read them from (a proof prefix per item)
int rsv_oods_eval(const uint32_t* samples4, const uint32_t* params26, uint32_t* out8, size_t n, int device) {
    if (n && (!samples4 || !params26 || !out8)) return RSV_E_NULL;
    if (n > ((size_t)1 << 20)) return RSV_E_SIZE;
    static constexpr SampleTable tab = make_sample_table();
    const size_t pw = tab.end;
    for (size_t i = 0; i < n * N_SAMPLES * 4; i++)
        if (samples4[i] >= RSV_M31_P) return RSV_E_RANGE;
    for (size_t i = 0; i < n; i++) {
        const uint32_t* pr = params26 + OODS_PARAM_WORDS * i;
        if (pr[0] < 1 || pr[0] > 28 || pr[1] < 1 || pr[1] > 28) return RSV_E_RANGE;
        for (int k = 2; k < (int)OODS_PARAM_WORDS; k++)
            if (pr[k] >= RSV_M31_P) return RSV_E_RANGE;
    }
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    if (n == 0) return RSV_OK;
    std::vector<uint32_t> prefix(n * pw, 0u);
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < N_SAMPLES; k++) memcpy(&prefix[i * pw + tab.off[k]], samples4 + (i * N_SAMPLES + k) * 4, 16);
    DevBuf dp, dpar, dout;
    HIP_TRY(dp.alloc(4 * prefix.size()));
    HIP_TRY(dpar.alloc(4 * OODS_PARAM_WORDS * n));
    HIP_TRY(dout.alloc(32 * n));
    HIP_TRY(hipMemcpy(dp.p, prefix.data(), 4 * prefix.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dpar.p, params26, 4 * OODS_PARAM_WORDS * n, hipMemcpyHostToDevice));
    launch_oods_probe(dp.as<const uint32_t>(), (uint32_t)pw, dpar.as<const uint32_t>(), dout.as<uint32_t>(), (uint32_t)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out8, dout.p, 32 * n, hipMemcpyDeviceToHost));
    return RSV_OK;
}

#ifdef RSV_COUNT_PERMS
// diagnostic build only: read and reset the permutation counters (not declared in rsv.h)
int rsv_debug_perm_counter(unsigned long long* out16) {
    unsigned long long zero[16] = {0};
    if (hipDeviceSynchronize() != hipSuccess) return RSV_E_DEVICE;
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_perm_counter), 128) != hipSuccess) return RSV_E_DEVICE;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_perm_counter), zero, 128) != hipSuccess) return RSV_E_DEVICE;
    return RSV_OK;
}

// diagnostic build only: run ONE of the two plan kernels on synthetic query sets (no proof behind them) and return its
// tables, so that tests can compare the kernels on shapes no fixture has (n_queries up to 128, duplicates, clusters).
//   raw_q [n][nq]; outputs: q_sorted [n][nq], qperm [n][nq] (u32), ent [n][(M+1)*G], fl [n][2*G], lvl [n][32], wf [n][32],
//   misc [n][8] = flags, n_sizes, sizes[0..2], fw_base[0..2]
int rsv_debug_plan(uint32_t n, uint32_t nq, uint32_t M, uint32_t A, uint32_t B, const uint32_t* raw_q, int serial,
                   uint32_t* q_sorted, uint32_t* qperm, uint32_t* ent, uint32_t* fl, uint32_t* lvl, uint32_t* wf, uint32_t* misc) {
    if (!raw_q || !q_sorted || !qperm || !ent || !fl || !lvl || !wf || !misc) return RSV_E_NULL;
    if (n == 0 || n > 4096 || nq == 0 || nq > (uint32_t)MAXQ || M == 0 || M > (uint32_t)MAX_LOG || A >= M || B >= M) return RSV_E_SIZE;
    const uint32_t G = nq < 4 ? 4u : nq;
    std::vector<ProofMeta> hm(n);
    std::vector<ProofCtx>* hc = new std::vector<ProofCtx>(n);
    memset(hm.data(), 0, sizeof(ProofMeta) * n);
    memset(hc->data(), 0, sizeof(ProofCtx) * n);
    for (uint32_t i = 0; i < n; i++) {
        hm[i].reason = R_OK; hm[i].nq = nq; hm[i].M = M; hm[i].A = A; hm[i].B = B; hm[i].first.wit_n = 0xFFFFFFFFu;
        memcpy((*hc)[i].raw_q, raw_q + (size_t)i * nq, 4 * nq);
    }
    DevBuf dm, dc, dh, de, df, dblob, doff;
    int rc = RSV_OK;
    const size_t ent_words = (size_t)n * (M + 1) * G, fl_words = (size_t)n * 2 * G;
    std::vector<uint64_t> offs(n + 1, 0);
    if (dm.alloc(sizeof(ProofMeta) * n) != hipSuccess || dc.alloc(sizeof(ProofCtx) * n) != hipSuccess ||
        dh.alloc(sizeof(PlanHdr) * n) != hipSuccess || de.alloc(4 * ent_words) != hipSuccess || df.alloc(4 * fl_words) != hipSuccess ||
        dblob.alloc(64) != hipSuccess || doff.alloc(8 * (n + 1)) != hipSuccess)
        rc = RSV_E_DEVICE;
    if (rc == RSV_OK && (hipMemcpy(dm.p, hm.data(), sizeof(ProofMeta) * n, hipMemcpyHostToDevice) != hipSuccess ||
                         hipMemcpy(dc.p, hc->data(), sizeof(ProofCtx) * n, hipMemcpyHostToDevice) != hipSuccess ||
                         hipMemcpy(doff.p, offs.data(), 8 * (n + 1), hipMemcpyHostToDevice) != hipSuccess ||
                         hipMemset(de.p, 0xEE, 4 * ent_words) != hipSuccess || hipMemset(df.p, 0xEE, 4 * fl_words) != hipSuccess ||
                         hipMemset(dh.p, 0, sizeof(PlanHdr) * n) != hipSuccess))
        rc = RSV_E_DEVICE;
    if (rc == RSV_OK) {
        PlanPtrs pl{};
        pl.hdr = dh.as<PlanHdr>(); pl.ent = de.as<uint32_t>(); pl.fl = df.as<uint32_t>(); pl.G = G; pl.maxM = M; pl.ids = nullptr; pl.p0 = 0;
        if (serial)
            hipLaunchKernelGGL(k_plan, dim3(grid_for(n, 64)), dim3(64), 0, 0, dblob.as<const uint8_t>(), doff.as<const uint64_t>(), n,
                               dm.as<const ProofMeta>(), dc.as<ProofCtx>(), pl);
        else
        {
            Fused<PlanArgs> fp{};
            fp.nb = 1;
            fp.first_block[0] = 0;
            fp.first_block[1] = (n + kBlock / G - 1) / (kBlock / G);
            fp.a[0] = PlanArgs{n, pl};
            fp.lds_proofs = kBlock / G;
            hipLaunchKernelGGL((k_plan_par<kBlock, false>), dim3(fp.first_block[1]), dim3(kBlock), plan_lds_bytes(kBlock / G), 0, dblob.as<const uint8_t>(),
                               doff.as<const uint64_t>(), dm.as<const ProofMeta>(), dc.as<ProofCtx>(), fp, 0u);
        }
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = RSV_E_DEVICE;
    }
    std::vector<PlanHdr> hh(n);
    if (rc == RSV_OK && (hipMemcpy(hc->data(), dc.p, sizeof(ProofCtx) * n, hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(hh.data(), dh.p, sizeof(PlanHdr) * n, hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(ent, de.p, 4 * ent_words, hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(fl, df.p, 4 * fl_words, hipMemcpyDeviceToHost) != hipSuccess))
        rc = RSV_E_DEVICE;
    if (rc == RSV_OK)
        for (uint32_t i = 0; i < n; i++) {
            const ProofCtx& c = (*hc)[i];
            for (uint32_t j = 0; j < nq; j++) { q_sorted[(size_t)i * nq + j] = c.q[j]; qperm[(size_t)i * nq + j] = c.qperm[j]; }
            for (uint32_t l = 0; l < 32; l++) { lvl[(size_t)i * 32 + l] = hh[i].lvl[l]; wf[(size_t)i * 32 + l] = hh[i].wf[l]; }
            uint32_t* ms = misc + (size_t)i * 8;
            ms[0] = c.flags; ms[1] = c.n_sizes; ms[2] = c.sizes[0]; ms[3] = c.sizes[1]; ms[4] = c.sizes[2];
            ms[5] = c.fw_base[0]; ms[6] = c.fw_base[1]; ms[7] = c.fw_base[2];
        }
    delete hc;
    return rc;
}
#endif

int rsv_last_stage_times(rsv_ctx* c, const char** names, float* ms, int cap) {
    if (!c || !names || !ms) return RSV_E_NULL;
    HIP_TRY(hipStreamSynchronize(c->stream));
    VerifyState* vs = state_of(c);
    int nst = cap < kNumStages ? cap : kNumStages;
    for (int i = 0; i < nst; i++) { names[i] = kStageNames[i]; ms[i] = 0.f; }
    for (auto& s : vs->spans) {
        if (!s.b || !s.e || s.stage >= nst) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, s.b, s.e) == hipSuccess) ms[s.stage] += t;
    }
    return nst;
}

int rsv_accept_bitmap_dev(rsv_ctx* c, const uint8_t* d_accept, size_t n, uint32_t* d_bitmap, uint64_t* d_count) {
    if (!c || (n && (!d_accept || !d_bitmap))) return RSV_E_NULL;
    if (n > (1u << 30)) return RSV_E_SIZE;
    HIP_TRY(hipSetDevice(c->device));
    if (d_count) HIP_TRY(hipMemsetAsync(d_count, 0, 8, c->stream));
    if (n == 0) return RSV_OK;
    hipLaunchKernelGGL(k_bitmap, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, d_accept, (uint32_t)n, d_bitmap,
                       reinterpret_cast<unsigned long long*>(d_count));
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

// Transcript parity probe: runs parse + transcript for one proof and returns
// the challenges (layout documented in include/rsv.h).
int rsv_transcript(const uint8_t* proof, size_t len, uint32_t* out, size_t cap, int device) {
    if (!proof || !out) return RSV_E_NULL;
    if (cap < 1) return RSV_E_CAP;
    if (len > (1u << 30)) return RSV_E_SIZE;
    int rc = select_device(device);
    if (rc != RSV_OK) return rc;
    DevBuf dblob, doffs, dmeta, dctx, dsum, dshape;
    uint64_t offs[2] = {0, len};
    HIP_TRY(dblob.alloc(len + 16));
    HIP_TRY(doffs.alloc(16));
    HIP_TRY(dmeta.alloc(sizeof(ProofMeta)));
    HIP_TRY(dctx.alloc(sizeof(ProofCtx)));
    HIP_TRY(dsum.alloc(256));
    HIP_TRY(dshape.alloc(16));
    HIP_TRY(hipMemset(dsum.p, 0, 256));
    HIP_TRY(hipMemcpy(dblob.p, proof, len, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(doffs.p, offs, 16, hipMemcpyHostToDevice));
    // probe: the configuration words serialized in the proof itself (documented in rsv.h: not a verdict)
    CfgSet co{};
    co.n = 1;
    if (len >= 4 * (W_NQ + 1)) {
        uint32_t hw[W_NQ + 1];
        memcpy(hw, proof, sizeof(hw));
        co.c[0][0] = hw[W_POW_BITS]; co.c[0][1] = hw[W_BLOWUP]; co.c[0][2] = hw[W_LOG_LAST]; co.c[0][3] = hw[W_NQ];
    }
    hipLaunchKernelGGL(k_parse, dim3(1), dim3(64), 0, 0, dblob.as<const uint8_t>(), doffs.as<const uint64_t>(), 1u, co,
                       dmeta.as<ProofMeta>(), dctx.as<ProofCtx>(), dsum.as<uint32_t>(), dshape.as<uint32_t>());
    // (the prefixes inside sampled_values are the OODS kernels' to check in the pipeline; no OODS evaluation runs here)
    hipLaunchKernelGGL(k_prefix_check, dim3(1), dim3(64), 0, 0, dblob.as<const uint8_t>(), doffs.as<const uint64_t>(), 1u,
                       dmeta.as<const ProofMeta>(), dctx.as<ProofCtx>());
    {
        const bool row = default_options().transcript_form != 2;
        if (row)
            hipLaunchKernelGGL(k_transcript_row<0>, dim3(1), dim3(256), 0, 0, dblob.as<const uint8_t>(), doffs.as<const uint64_t>(),
                               1u, dmeta.as<const ProofMeta>(), dctx.as<ProofCtx>(), FlowArgs{nullptr, nullptr, nullptr, 0});
        else
            hipLaunchKernelGGL(k_transcript<false>, dim3(1), dim3(64), 0, 0, dblob.as<const uint8_t>(), doffs.as<const uint64_t>(), 1u,
                               dmeta.as<const ProofMeta>(), dctx.as<ProofCtx>(), FlowArgs{nullptr, nullptr, nullptr, 0});
    }
    // no Merkle stage runs here: the whole proof is read for canonicity (k_finalize, force)
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, 0, dblob.as<const uint8_t>(), doffs.as<const uint64_t>(), 1u,
                       dmeta.as<const ProofMeta>(), dctx.as<ProofCtx>(), (uint8_t*)nullptr, (uint8_t*)nullptr, 1u, (uint32_t*)nullptr,
                       (unsigned long long*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    std::vector<char> hm(sizeof(ProofMeta)), hc(sizeof(ProofCtx));
    HIP_TRY(hipMemcpy(hm.data(), dmeta.p, sizeof(ProofMeta), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hc.data(), dctx.p, sizeof(ProofCtx), hipMemcpyDeviceToHost));
    const ProofMeta* m = reinterpret_cast<const ProofMeta*>(hm.data());
    const ProofCtx* x = reinterpret_cast<const ProofCtx*>(hc.data());
    if (m->reason != R_OK || (x->flags & (1u << R_PARSE))) { out[0] = RSV_R_PARSE; return RSV_OK; }
    size_t need = 40 + 4 * (size_t)(m->n_inner + 1) + m->nq;
    if (cap < need) return RSV_E_CAP;
    out[0] = (x->flags & (1u << R_POW)) ? RSV_R_POW : RSV_R_OK;
    out[1] = m->n_inner + 1; out[2] = m->nq; out[3] = m->M;
    memcpy(out + 4, x->z, 16); memcpy(out + 8, x->alpha, 16); memcpy(out + 12, x->rc, 16);
    memcpy(out + 16, x->oods_t, 16); memcpy(out + 20, x->oods_x, 16); memcpy(out + 24, x->oods_y, 16);
    memcpy(out + 28, x->after, 16); memcpy(out + 32, x->pow_digest, 32);
    memcpy(out + 40, x->fri_alpha, 16 * (m->n_inner + 1));
    memcpy(out + 40 + 4 * (m->n_inner + 1), x->raw_q, 4 * m->nq);
    return RSV_OK;
}

}  // extern "C"
