// verify_api.inc — host launcher of the verify pipeline (included by rsv_hip.hip).  Every decision that touches no device
// lives in host_logic.hpp, where a sanitizer can reach it: the shape buckets, the workspace groups, and the launch plan
// (VerifyPlan) — which form of each kernel a batch runs and on which stream.  verify_impl checks its arguments, builds the
// plan and then only enqueues, stage function by stage function; none of them decides a form, each reads the plan.
// The host-pointer forms behind it (rsv_verify_batch, _inputs, _hints, the probes) stage through host_stage.inc.
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

using rsv::host::kBlock;
using rsv::host::kRowTreeBlock;
using rsv::host::Bucket;
using rsv::host::Carve;
using rsv::host::Entry;

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

// the OODS evaluation's two forms (host_logic.hpp: oods_row_form): one proof per 16-lane row, or one proof per lane
static void launch_oods_probe(const uint32_t* d_prefix, uint32_t prefix_words, const uint32_t* d_params, uint32_t* d_out, uint32_t n) {
    const bool row = rsv::host::oods_row_form(default_options(), n);
    const unsigned block = row ? 256 : 64;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid_for((size_t)n * (row ? 16 : 1), block)), dim3(block), 0, 0, d_prefix, prefix_words, d_params, d_out, n);
    };
    row ? launch(k_oods_row_probe) : launch(k_oods_probe);
}

namespace {
// One verify call, as its stage functions share it: the context, the arguments, the plan (host_logic.hpp), the records
// carved out of the fixed workspace, what one stage leaves for the next, and the stage clock.
struct VerifyCall {
    rsv_ctx* c;
    hipStream_t st;  // the main stream (the other two: c->side, c->aux)
    VerifyState* vs;
    const uint8_t* d_blob;
    const uint64_t* d_offsets;
    uint32_t N;
    CfgSet co;
    size_t n_pi;
    // nullptr — the batch's one table, copied to c->d_pi; else [n][n_pi] records in HBM, every proof its own: k_pi_sum
    // sums them per proof and the OODS kernel reads that sum (k_pi_sum.hpp)
    const rsv_public_input* d_own_pi;
    uint8_t *d_accept, *d_reason;
    const PathsOut* po;
    FlowArgs fargs;
    rsv::host::PlanInputs in;
    rsv::host::VerifyPlan plan;
    // whole-batch records (ws_fixed)
    uint32_t* summary;
    ProofMeta* metas;
    ProofCtx* ctxs;
    uint32_t *d_shape, *d_ids;
    ClassTable* d_classes;
    uint8_t* d_cls;
    uint32_t* d_pi_sum;  // k_pi_sum -> k_oods<PiOwn>
    // the slot order: shape buckets, one launch geometry per distinct n_queries (host_logic.hpp)
    bool live;     // some proof has a lane somewhere
    bool uniform;  // one bucket in natural order: no slot -> proof list
    std::vector<Bucket> buckets;
    // the row hashes, addressed by slot: where each bucket's begin
    uint32_t* rowh;
    std::vector<size_t> row_base;
    bool joined;  // the main stream has waited for the row hashes

    // Stage clock: opt-in (RSV_OPT_STAGE_TIMES).  Two event records around a stage cost ~8 us of queue time EACH STAGE
    // (tools/chain_lab.hip: 5.3 us per dependent empty launch, 13.3 with the two records) — on a small batch's chain of
    // seven stages that was 4 % of the call, paid by every caller for a diagnostic only bench.py reads.
    bool timing;
    void begin_on(int stage, hipStream_t on) {
        if (!timing) return;
        hipEvent_t b = vs->clock.next();
        if (b) (void)hipEventRecord(b, on);
        vs->spans.push_back({stage, b, nullptr});
    }
    void end_on(hipStream_t on) {
        if (!timing) return;
        hipEvent_t e = vs->clock.next();
        if (e) (void)hipEventRecord(e, on);
        for (size_t i = vs->spans.size(); i-- > 0;)  // the span opened last and not yet closed
            if (!vs->spans[i].e) { vs->spans[i].e = e; break; }
    }
};
}  // namespace

// Stages 1 and 2: the parser and the transcript.
static int enqueue_parse_transcript(VerifyCall& v) {
    rsv_ctx* c = v.c;
    hipStream_t st = v.st;
    const uint32_t N = v.N;
    const bool row = v.plan.transcript_row, split = v.plan.transcript_split, flow = v.in.flow;
    if (flow && v.fargs.count) HIP_TRY(hipMemsetAsync(v.fargs.count, 0, sizeof(uint32_t) * (size_t)N, st));
    // Split: the PARSER goes to the aux stream and the front half stays on the main stream, in front of the back half — the
    // parser (0.04-0.1 ms) is long over when the front half (0.16-0.19 ms) ends, so the back half's wait for it is a wait
    // for an event signalled long ago, and front -> back is a boundary inside one stream (~5 us) instead of a fresh
    // cross-stream wait (15 us; until the end of round 4 the front half was the one on the aux stream).
    hipStream_t parse_on = split ? c->aux : st;
    if (split) {
        HIP_TRY(hipEventRecord(c->ev_begin, st));  // behind whatever produced the blob, the offsets and the inputs
        HIP_TRY(hipStreamWaitEvent(c->aux, c->ev_begin, 0));
    }
    v.begin_on(0, parse_on);
    HIP_TRY(hipMemsetAsync(v.summary, 0, 256, parse_on));
    hipLaunchKernelGGL(k_parse, dim3(grid_for(N, 64)), dim3(64), 0, parse_on, v.d_blob, v.d_offsets, N, v.co, v.metas, v.ctxs, v.summary, v.d_shape);
    v.end_on(parse_on);
    HIP_TRY(hipGetLastError());
    // The transcript needs nothing from the host: it is enqueued right behind the parser, and the parse summary
    // (and, for mixed batches, the shape words) travel back through the side stream while it runs.
    HIP_TRY(hipEventRecord(c->ev_fork, parse_on));
    const unsigned block = row ? 256 : 64;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid_for((size_t)N * (row ? 16 : 1), block)), dim3(block), 0, st, v.d_blob, v.d_offsets, N, v.metas, v.ctxs, v.fargs);
    };
    if (split) {
        launch(k_transcript_row<1>);
        HIP_TRY(hipStreamWaitEvent(st, c->ev_fork, 0));  // everything behind this on the main stream may read the parser's tables
    }
    v.begin_on(1, st);
    if (split) launch(k_transcript_row<2>);
    else if (row) flow ? launch(k_transcript_row<0, true>) : launch(k_transcript_row<0>);
    else if (flow) launch(k_transcript<true>);
    else !v.plan.transcript_paced ? launch(k_transcript<false, false>) : launch(k_transcript<false, true>);
    v.end_on(st);
    HIP_TRY(hipEventRecord(c->ev_tr, st));
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

// Stage 3: the slot order and the shape buckets — on the device with nothing read back (the plan's device_order), or from
// the parse summary on the host.  RSV_E_SIZE: path outputs were asked for and the batch is not of the one declared shape.
static int enqueue_slot_order(VerifyCall& v) {
    rsv_ctx* c = v.c;
    const uint32_t N = v.N;
    const PathsOut* po = v.po;
    const bool device_order = v.plan.device_order;
    uint32_t sum[8] = {0};
    HIP_TRY(hipStreamWaitEvent(c->side, c->ev_fork, 0));
    if (device_order) {
        HIP_TRY(hipMemsetAsync(v.d_classes, 0, sizeof(ClassTable), c->side));
        hipLaunchKernelGGL(k_classify, dim3(grid_for(N, CLASSIFY_PER_BLOCK)), dim3(256), 0, c->side, N, v.d_shape, v.d_classes, v.d_cls);
        hipLaunchKernelGGL(k_class_offsets, dim3(1), dim3(64), 0, c->side, v.d_classes);
        hipLaunchKernelGGL(k_scatter_ids, dim3(grid_for(N, 256)), dim3(256), 0, c->side, N, v.d_cls, v.d_classes, v.d_ids);
        sum[0] = 1;
    } else {
        HIP_TRY(hipMemcpyAsync(sum, v.summary, 32, hipMemcpyDeviceToHost, c->side));
        HIP_TRY(hipStreamSynchronize(c->side));
    }
    v.live = sum[0] > 0;
    if (!v.live) return RSV_OK;
    v.uniform = !device_order && sum[4] == ~sum[5] && sum[6] == ~sum[7];
    if (device_order) {
        // every slot of the batch (rejected proofs have no live lane), the deepest trees the parser admits
        const uint32_t b = v.co.c[0][1], last = v.co.c[0][2];
        const uint32_t inner_bound = (uint32_t)MAX_LOG - 1u - (last + b);
        v.buckets.push_back({v.co.c[0][3], (uint32_t)MAX_LOG, inner_bound > (uint32_t)MAX_INNER ? (uint32_t)MAX_INNER : inner_bound, last + b + 1u, N, 0});
    } else if (po && po->paths() && (!v.uniform || (sum[4] & 0xFFu) != po->n_queries || ((sum[4] >> 8) & 0xFFu) != po->max_log || po->n_queries < 4 ||
                                     ((po->d_pair_sib || po->d_pair_cols || po->d_qv) && ((sum[4] >> 16) & 0xFFu) != po->n_inner))) {
        return RSV_E_SIZE;  // path emission needs one shape for the whole batch, as declared by the caller
    } else if (v.uniform) {
        v.buckets.push_back({sum[4] & 0xFFu, (sum[4] >> 8) & 0xFFu, (sum[4] >> 16) & 0xFFu, sum[4] >> 24, N, 0});
    } else {
        // Mixed batch: 8 bytes per proof come back, the host buckets them (rsv::host::bucket_by_shape) and uploads the
        // slot -> proof list.
        std::vector<uint32_t>& shape = v.vs->h_shape;
        shape.resize(2 * (size_t)N);
        HIP_TRY(hipMemcpyAsync(shape.data(), v.d_shape, 8 * (size_t)N, hipMemcpyDeviceToHost, c->side));
        HIP_TRY(hipStreamSynchronize(c->side));
        std::vector<uint32_t>& ids = v.vs->h_ids;
        rsv::host::bucket_by_shape(shape.data(), N, v.buckets, ids, v.vs->h_class);
        if (!ids.empty()) HIP_TRY(hipMemcpyAsync(v.d_ids, ids.data(), 4 * ids.size(), hipMemcpyHostToDevice, c->side));
    }
    // the slot -> proof list was uploaded on the side stream: k_plan (main stream) waits for it
    HIP_TRY(hipEventRecord(c->ev_ids, c->side));
    HIP_TRY(hipStreamWaitEvent(v.st, c->ev_ids, 0));
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

// Side stream: trace-tree column hashing (independent of the transcript), so that it fills the issue slots the
// one-wave-per-SIMD transcript kernel leaves idle.  Row hashes are addressed by SLOT and sized per bucket
// (count x that bucket's n_queries): one well-formed 128-query header in a batch of 16-query proofs must not
// inflate the allocation of the whole batch.  All buckets go into ONE launch (Fused<>, at most MAX_FUSED each).
static int enqueue_row_hashes(VerifyCall& v) {
    rsv_ctx* c = v.c;
    const std::vector<Bucket>& buckets = v.buckets;
    v.row_base.resize(buckets.size());
    size_t row_words = 0;
    for (size_t bi = 0; bi < buckets.size(); bi++) {
        v.row_base[bi] = row_words;
        row_words += (size_t)buckets[bi].count * 4 * 2 * rsv::host::padded_lanes(buckets[bi]) * 8;
    }
    const int rc = ensure_buf(c, &c->ws_rows, &c->ws_rows_bytes, row_words * 4);
    if (rc != RSV_OK) return rc;
    v.rowh = static_cast<uint32_t*>(c->ws_rows);
    v.begin_on(9, c->side);
    for (size_t b0 = 0; b0 < buckets.size(); b0 += MAX_FUSED) {
        Fused<RowHashArgs> fr{};
        uint32_t blocks = 0;
        for (size_t bi = b0; bi < buckets.size() && bi < b0 + MAX_FUSED; bi++) {
            const Bucket& b = buckets[bi];
            const uint32_t gq = rsv::host::padded_lanes(b);
            fr.first_block[fr.nb] = blocks;
            fr.a[fr.nb++] = RowHashArgs{v.d_blob, v.d_offsets, b.count, gq, v.metas, v.rowh + v.row_base[bi], v.uniform ? nullptr : v.d_ids + b.first, v.ctxs};
            blocks += grid_for((size_t)b.count * gq, kBlock);
        }
        fr.first_block[fr.nb] = blocks;
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(blocks, 4), dim3(kBlock), 0, c->side, fr); };
        v.plan.small_trees ? launch(k_row_hash<false>) : launch(k_row_hash<true>);
    }
    v.end_on(c->side);
    HIP_TRY(hipEventRecord(c->ev_join, c->side));
    return RSV_OK;
}

// the row form of the quotient constants, in k_qconst_row or inside the plan's launch: its workgroups, and its proof count
// with the four-rows-per-proof flag
static unsigned qconst_row_blocks(const VerifyCall& v) { return grid_for((size_t)v.N * (v.plan.qconst4 ? 64 : 16), 256); }
static uint32_t qconst_row_n(const VerifyCall& v) { return v.N | (v.plan.qconst4 ? 0x80000000u : 0u); }

// query-independent quotient constants: need only the transcript
static void launch_qconst(VerifyCall& v, hipStream_t on) {
    v.begin_on(10, on);
    if (v.plan.qconst_row)
        hipLaunchKernelGGL(k_qconst_row, dim3(qconst_row_blocks(v)), dim3(256), 0, on, v.d_blob, v.d_offsets, qconst_row_n(v), v.metas, v.ctxs);
    else
        hipLaunchKernelGGL(k_qconst, dim3(grid_for(v.N, 64)), dim3(64), 0, on, v.d_blob, v.d_offsets, v.N, v.metas, v.ctxs);
    v.end_on(on);
}

// Stage 5: the OODS composition check, behind the transcript on whichever stream the plan puts it.
static void launch_oods(VerifyCall& v, hipStream_t on) {
    const uint32_t N = v.N;
    const bool row = v.plan.oods_row, own = v.in.own;
    v.begin_on(2, on);
    const PiShared shared{reinterpret_cast<const PubInput*>(v.c->d_pi), (uint32_t)v.n_pi};
    const PiOwn sums{v.d_pi_sum};
    // per-proof inputs: the statement sums first, on the same stream (behind the transcript, as the OODS kernel is)
    if (own)
        hipLaunchKernelGGL(k_pi_sum<true>, dim3(grid_for(N, PI_WAVES)), dim3(64 * PI_WAVES), 0, on, reinterpret_cast<const uint32_t*>(v.d_own_pi),
                           N, (uint32_t)v.n_pi, v.metas, v.ctxs, (const uint32_t*)nullptr, v.d_pi_sum, (uint8_t*)nullptr);
    const unsigned block = row ? 256 : 64;
    auto launch = [&](auto kernel, auto inputs) {
        hipLaunchKernelGGL(kernel, dim3(grid_for((size_t)N * (row ? 16 : 1), block)), dim3(block), 0, on, v.d_blob, v.d_offsets, N, v.metas, v.ctxs, inputs);
    };
    if (row) own ? launch(k_oods_row<PiOwn>, sums) : launch(k_oods_row<PiShared>, shared);
    else own ? launch(k_oods<PiOwn>, sums) : launch(k_oods<PiShared>, shared);
    v.end_on(on);
}

namespace {
// The launches of one group: the argument tables of its entries (a group is ONE launch per stage) and their grids.
struct GroupLaunch {
    Fused<PlanArgs> fp;
    Fused<QueryArgs> fq;
    Fused<MerkleArgs> fm;
    CapTopIndex ix_t, ix_p, ix_mt, ix_mp;  // k_cap_top / k_cap_mid over the trace (t) and the FRI (p) trees
    uint32_t blocks, blocks_m, blocks_q;   // workgroups of kBlock lanes / of the tree kernels / of k_query's row form
    uint32_t max_inner, top_t, top_p, mid_t, mid_p;
    bool any_top, any_mid;
    rsv::host::GroupPlan plan;
};
}  // namespace

// carves the group's workspace (the groups share c->ws) and fills the argument tables
static void fill_group(VerifyCall& v, const std::vector<Entry>& grp, GroupLaunch& g) {
    const PathsOut* po = v.po;
    const bool query_row = v.plan.query_row;
    const uint32_t row_lanes = (uint32_t)kRowTreeBlock / 16u;
    Carve wq{static_cast<char*>(v.c->ws)};
    uint32_t pbmax = 1;
    for (const Entry& en : grp) {
        const Bucket& b = v.buckets[en.bi];
        PlanPtrs pl{};
        pl.hdr = wq.take<PlanHdr>(en.cn);
        pl.ent = wq.take<uint32_t>((size_t)en.cn * (b.maxM + 1) * en.G);
        pl.fl = wq.take<uint32_t>((size_t)en.cn * 2 * en.G);
        pl.G = en.G;
        pl.maxM = b.maxM;
        uint32_t* leafv = wq.take<uint32_t>((size_t)en.cn * (3 + b.maxInner) * en.G * 8);
        pl.ids = v.uniform ? nullptr : v.d_ids + b.first + en.c0;
        pl.p0 = v.uniform ? (uint32_t)en.c0 : 0u;
        const size_t c0 = en.c0;
        QueryArgs qa{v.d_blob, v.d_offsets, en.cn, v.metas, v.ctxs, pl, leafv, b.maxInner,
                     (po && po->d_folded) ? po->d_folded + c0 * 3 * en.G * 4 : nullptr,
                     (po && po->d_qv) ? po->d_qv + c0 * en.G * 4 * (8 + b.maxInner) : nullptr, 4 * (8 + b.maxInner)};
        MerkleArgs ma{v.d_blob, v.d_offsets, en.cn, v.metas, v.ctxs, pl, leafv, b.maxInner, en.Lc,
                      v.rowh + v.row_base[en.bi] + c0 * 4 * 2 * (size_t)en.G * 8, nullptr, nullptr, nullptr, nullptr, nullptr,
                      en.Lt, en.Lt2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (en.Lt) {
            ma.tcapn = wq.take<uint32_t>(((size_t)en.cn * 4 << en.Lt) * 8);
            ma.tcapm = wq.take<unsigned long long>((size_t)en.cn * 4);
            ma.pcapn = wq.take<uint32_t>(((size_t)en.cn * (1 + b.maxInner) << en.Lt) * 8);
            ma.pcapm = wq.take<unsigned long long>((size_t)en.cn * (1 + b.maxInner));
            g.any_top = true;
        }
        if (en.Lt2 != en.Lt) {  // the levels between the hand-over and k_cap_top's: k_cap_mid
            ma.tcapn2 = wq.take<uint32_t>(((size_t)en.cn * 4 << en.Lt2) * 8);
            ma.tcapm2 = wq.take<unsigned long long>((size_t)en.cn * 4);
            ma.pcapn2 = wq.take<uint32_t>(((size_t)en.cn * (1 + b.maxInner) << en.Lt2) * 8);
            ma.pcapm2 = wq.take<unsigned long long>((size_t)en.cn * (1 + b.maxInner));
            g.any_mid = true;
        }
        if (po && po->d_sib) {
            ma.path_sib = po->d_sib + c0 * 4 * en.G * b.maxM * 8;
            ma.path_pos = po->d_pos + c0 * 4 * en.G;
        }
        if (po && po->d_cols) ma.path_cols = po->d_cols + c0 * 4 * en.G * 64;
        if (po && po->d_pair_sib) ma.pair_sib = po->d_pair_sib + c0 * (1 + b.maxInner) * en.G * b.maxM * 8;
        if (po && po->d_pair_cols) ma.pair_cols = po->d_pair_cols + c0 * (1 + b.maxInner) * en.G * 3 * 8;
        const uint32_t k = g.fp.nb;
        g.fp.first_block[k] = g.blocks;
        g.fq.first_block[k] = query_row ? g.blocks_q : g.blocks;
        g.fm.first_block[k] = g.blocks_m;
        g.ix_t.first_block[k] = g.top_t;
        g.ix_p.first_block[k] = g.top_p;
        g.top_t += grid_for((size_t)en.cn * 4, 256);
        g.top_p += grid_for((size_t)en.cn * (1 + b.maxInner), 256);
        g.ix_mt.first_block[k] = g.mid_t;
        g.ix_mp.first_block[k] = g.mid_p;
        if (en.Lt2 != en.Lt) {
            g.mid_t += grid_for((size_t)en.cn * 4 << en.Lt2, 256);
            g.mid_p += grid_for((size_t)en.cn * (1 + b.maxInner) << en.Lt2, 256);
        }
        g.fp.a[k] = PlanArgs{en.cn, pl};
        g.fq.a[k] = qa;
        g.fm.a[k] = ma;
        g.fp.nb = g.fq.nb = g.fm.nb = k + 1;
        const uint32_t per_block = kBlock / en.G, per_block_m = v.plan.tree_lanes / en.G;
        g.blocks += (en.cn + per_block - 1) / per_block;
        g.blocks_m += (en.cn + per_block_m - 1) / per_block_m;
        if (query_row) g.blocks_q += (en.cn + row_lanes / en.G - 1) / (row_lanes / en.G);
        g.max_inner = std::max(g.max_inner, b.maxInner);
        pbmax = std::max<uint32_t>(pbmax, kBlock / en.G);
    }
    g.fp.lds_proofs = pbmax;  // (k_plan_par's LDS; the serial k_plan does not see the table)
    g.fp.first_block[g.fp.nb] = g.blocks;
    g.fq.first_block[g.fq.nb] = query_row ? g.blocks_q : g.blocks;
    g.fm.first_block[g.fm.nb] = g.blocks_m;
    g.ix_t.first_block[g.fm.nb] = g.top_t;
    g.ix_p.first_block[g.fm.nb] = g.top_p;
    g.ix_mt.first_block[g.fm.nb] = g.mid_t;
    g.ix_mp.first_block[g.fm.nb] = g.mid_p;
    g.plan = rsv::host::plan_group(v.plan, v.in, v.buckets, grp);
    // which FRI tree each grid row of k_pair_merkle hashes: dealt out over the compute units for a launch that is
    // resident all at once (host_logic.hpp), the identity otherwise (and with RSV_OPT_PAIR_ORDER = 2)
    for (uint32_t k = 0; k < 32; k++) g.fm.y_of[k] = (uint8_t)k;
    if (v.plan.pair_deal)
        rsv::host::pair_layer_order(g.blocks_m, 1 + g.max_inner, g.plan.live, g.plan.group_M, (uint32_t)v.c->n_cu, (uint32_t)RSV_PAIR_WAVES, g.fm.y_of);
}

static void launch_plan(VerifyCall& v, const GroupLaunch& g) {
    v.begin_on(3, v.st);
    if (v.plan.serial_plan) {
        for (uint32_t k = 0; k < g.fp.nb; k++)
            hipLaunchKernelGGL(k_plan, dim3(grid_for(g.fp.a[k].n, 64)), dim3(64), 0, v.st, v.d_blob, v.d_offsets, g.fp.a[k].n, v.metas, v.ctxs, g.fp.a[k].pl);
    } else {
        // the row-form quotient constants of a chain-layout batch ride in the plan's launch: their workgroups behind the plan's
        auto launch = [&](auto kernel, unsigned qconst_blocks, uint32_t qconst_n) {
            hipLaunchKernelGGL(kernel, dim3(g.blocks + qconst_blocks), dim3(kBlock), plan_lds_bytes(g.fp.lds_proofs), v.st, v.d_blob, v.d_offsets, v.metas,
                               v.ctxs, g.fp, qconst_n);
        };
        v.plan.qconst_in_plan ? launch(k_plan_par<kBlock, true>, qconst_row_blocks(v), qconst_row_n(v)) : launch(k_plan_par<kBlock, false>, 0u, 0u);
    }
    v.end_on(v.st);
}

static void launch_pair_merkle(VerifyCall& v, const GroupLaunch& g, hipStream_t on) {
    const int form = v.plan.tree_form;
    v.begin_on(6, on);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(g.blocks_m, 1 + g.max_inner), dim3(form == 2 ? kRowTreeBlock : kBlock), g.plan.pair_lds, on, g.fm, v.fargs);
    };
    if (v.in.flow) form == 2 ? launch(k_pair_merkle<kRowTreeBlock, true, FORM_ROW>) : launch(k_pair_merkle<kBlock, true>);
    else if (form == 2) launch(k_pair_merkle<kRowTreeBlock, false, FORM_ROW>);
    else form == 0 ? launch(k_pair_merkle<kBlock, false, 0>) : launch(k_pair_merkle<kBlock, false, 1>);
    v.end_on(on);
}

static void launch_trace_merkle(VerifyCall& v, const GroupLaunch& g, hipStream_t on) {
    const int form = v.plan.tree_form;
    v.begin_on(5, on);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(g.blocks_m, 4), dim3(form == 2 ? kRowTreeBlock : kBlock), 0, on, g.fm, v.fargs); };
    if (v.in.flow) form == 2 ? launch(k_trace_merkle<kRowTreeBlock, true, FORM_ROW>) : launch(k_trace_merkle<kBlock, true>);
    else if (form == 2) launch(k_trace_merkle<kRowTreeBlock, false, FORM_ROW>);
    else form == 0 ? launch(k_trace_merkle<kBlock, false, 0>) : launch(k_trace_merkle<kBlock, false, 1>);
    v.end_on(on);
}

// the last levels of the trees of a kernel, right behind it on its stream (stage 8)
static void launch_cap(VerifyCall& v, const GroupLaunch& g, hipStream_t on, bool pair) {
    if (!g.any_top) return;
    v.begin_on(8, on);
    // (fast: a small batch's few waves: the permutation instance without wait states, as the tree kernels in front of it)
    const bool tm = pair ? g.plan.tm_p : g.plan.tm_t, fast = v.plan.tree_form == 0;
    const uint32_t mid = pair ? g.mid_p : g.mid_t, top = pair ? g.top_p : g.top_t;
    auto launch = [&](auto kernel, uint32_t blocks, const CapTopIndex& ix) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, on, g.fm, ix, pair ? 1u : 0u); };
    if (g.any_mid && mid) {  // buckets that hand over at the cap level: the levels down to k_cap_top's first
        const CapTopIndex& ix = pair ? g.ix_mp : g.ix_mt;
        if (fast) tm ? launch(k_cap_mid<0, true>, mid, ix) : launch(k_cap_mid<0, false>, mid, ix);
        else tm ? launch(k_cap_mid<1, true>, mid, ix) : launch(k_cap_mid<1, false>, mid, ix);
    }
    const CapTopIndex& ix = pair ? g.ix_p : g.ix_t;
    if (fast) tm ? launch(k_cap_top<0, true>, top, ix) : launch(k_cap_top<0, false>, top, ix);
    else tm ? launch(k_cap_top<1, true>, top, ix) : launch(k_cap_top<1, false>, top, ix);
    v.end_on(on);
}

// (behind the tree kernels in this file: the library keeps its kernels in the order of their first mention)
static void launch_query(VerifyCall& v, const GroupLaunch& g, hipStream_t on) {
    const bool row = v.plan.query_row;  // a row of 16 threads per query
    v.begin_on(4, on);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(row ? g.blocks_q : g.blocks), dim3(row ? kRowTreeBlock : kBlock), 0, on, g.fq); };
    if (row) launch(k_query<kRowTreeBlock, 4, true>);
    else v.plan.chain ? launch(k_query<kBlock, 4>) : launch(k_query<kBlock, 2>);  // chain layout = small batch: the latency form
    v.end_on(on);
}

// Stage 4, one group.  k_plan needs only the transcript, k_trace_merkle needs the plan and the row hashes, k_query
// (quotients + folds) is needed only by k_pair_merkle.
static int enqueue_group(VerifyCall& v, const std::vector<Entry>& grp) {
    rsv_ctx* c = v.c;
    hipStream_t st = v.st;
    GroupLaunch g{};
    fill_group(v, grp, g);
    launch_plan(v, g);
    HIP_TRY(hipEventRecord(c->ev_plan, st));
    HIP_TRY(hipStreamWaitEvent(c->side, c->ev_plan, 0));
    if (v.plan.chain) {
        // side: trace trees behind the row hashes (same stream) and the plan (event); main: k_query, FRI trees
        launch_trace_merkle(v, g, c->side);
        launch_cap(v, g, c->side, false);
        launch_query(v, g, st);
        launch_pair_merkle(v, g, st);
        launch_cap(v, g, st, true);
        HIP_TRY(hipGetLastError());
        return RSV_OK;
    }
    // k_query on the side stream underneath k_trace_merkle
    launch_query(v, g, c->side);
    HIP_TRY(hipEventRecord(c->ev_query, c->side));
    if (!v.joined) { HIP_TRY(hipStreamWaitEvent(st, c->ev_join, 0)); v.joined = true; }
    if (v.plan.overlap_trees) {
        launch_pair_merkle(v, g, c->side);
        launch_cap(v, g, c->side, true);
    }
    launch_trace_merkle(v, g, st);
    if (v.plan.oods_on_main) launch_oods(v, st);  // in front of the trace trees' last levels: underneath the FRI trees
    launch_cap(v, g, st, false);
    if (!v.plan.overlap_trees) {
        HIP_TRY(hipStreamWaitEvent(st, c->ev_query, 0));
        launch_pair_merkle(v, g, st);
        launch_cap(v, g, st, true);
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

// Stages 4 and 5.  The batch is cut into GROUPS of at most MAX_FUSED (bucket, slot range) entries whose workspaces fit the
// budget together; a group is ONE launch per stage.  A uniform batch is one entry (several groups only when it exceeds
// the budget), a mixed batch normally one group with an entry per n_queries.
static int enqueue_query_stages(VerifyCall& v) {
    rsv_ctx* c = v.c;
    std::vector<std::vector<Entry>> groups;
    const size_t need = rsv::host::plan_groups(v.buckets, v.plan.policy, groups);
    int rc = ensure_buf(c, &c->ws, &c->ws_bytes, need);
    if (rc != RSV_OK) return rc;
    rsv::host::plan_launches(v.plan, c->opt, v.in, groups);
    if (!v.plan.qconst_in_plan) {
        if (v.plan.chain) launch_qconst(v, v.st);
        else {
            HIP_TRY(hipStreamWaitEvent(c->side, c->ev_tr, 0));
            launch_qconst(v, c->side);
        }
    }
    for (const std::vector<Entry>& grp : groups) {
        rc = enqueue_group(v, grp);
        if (rc != RSV_OK) return rc;
    }
    if (!v.plan.oods_on_main) launch_oods(v, c->side);
    HIP_TRY(hipEventRecord(c->ev_scan, c->side));
    return RSV_OK;
}

// Stage 6: verdicts (+ the canonicity fallback for proofs whose witness lists some stage found of the wrong length, + the
// accept bitmap when the caller asked for it): ONE launch behind the Merkle stages
static int enqueue_finalize(VerifyCall& v) {
    const PathsOut* po = v.po;
    if (v.live) HIP_TRY(hipStreamWaitEvent(v.st, v.c->ev_scan, 0));
    v.begin_on(7, v.st);
    hipLaunchKernelGGL(k_finalize, dim3(grid_for(v.N, 256)), dim3(256), 0, v.st, v.d_blob, v.d_offsets, v.N, v.metas, v.ctxs, v.d_accept, v.d_reason, 0u,
                       po ? po->d_bitmap : nullptr, reinterpret_cast<unsigned long long*>(po ? po->d_count : nullptr));
    v.end_on(v.st);
    if (po && po->d_transcript)  // behind every stage that can find a non-canonical word: such a proof's row says RSV_R_PARSE
        hipLaunchKernelGGL(k_export_transcript, dim3(grid_for((size_t)v.N * TR_WORDS, 256)), dim3(256), 0, v.st, v.N, v.metas, v.ctxs, po->d_transcript);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

// The shared table of public inputs, the outputs that start from zero, and the whole-batch records.
static int enqueue_inputs(VerifyCall& v, const rsv_public_input* pi) {
    rsv_ctx* c = v.c;
    hipStream_t st = v.st;
    const PathsOut* po = v.po;
    const uint32_t N = v.N;
    const size_t n_pi = v.n_pi;
    const bool own = v.in.own;
    if (c->d_pi_cap < n_pi + 1) {
        if (c->d_pi) (void)hipFree(c->d_pi);
        c->d_pi = nullptr;
        c->d_pi_cap = 0;
        HIP_TRY(hipMalloc((void**)&c->d_pi, sizeof(rsv_public_input) * (n_pi + 16)));
        c->d_pi_cap = n_pi + 16;
    }
    if (c->opt.ws_fill) {  // in front of the copy (the shared table) or of nothing (per-proof inputs never read it)
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
    const size_t pi_sum_words = own ? 4 * (size_t)N : 0;
    auto carve_fixed = [&](Carve& cv) {
        v.summary = cv.take<uint32_t>(64);
        v.metas = cv.take<ProofMeta>(N);
        v.ctxs = cv.take<ProofCtx>(N);
        v.d_shape = cv.take<uint32_t>(2 * (size_t)N);
        v.d_ids = cv.take<uint32_t>(N);
        v.d_classes = cv.take<ClassTable>(1);
        v.d_cls = cv.take<uint8_t>(N);
        v.d_pi_sum = cv.take<uint32_t>(pi_sum_words);
    };
    Carve probe{nullptr};
    carve_fixed(probe);
    const int rc = ensure_buf(c, &c->ws_fixed, &c->ws_fixed_bytes, probe.off);
    if (rc != RSV_OK) return rc;
    Carve cv{static_cast<char*>(c->ws_fixed)};
    carve_fixed(cv);
    c->last_metas = v.metas;
    return RSV_OK;
}

static int verify_impl(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                       const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, const rsv_public_input* d_own_pi,
                       uint8_t* d_accept, uint8_t* d_reason, const PathsOut* po) {
    // d_own_pi: nullptr — `pi` is the batch's one table, in host memory; else [n][n_pi] records in HBM, every proof its own
    // (`pi` is unused)
    if (!c) return RSV_E_NULL;
    VerifyCall v{};
    {
        int rc0 = make_cfg_set(cfg, &v.co);  // required even for an empty batch: a caller that forgot it learns at once
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
    const uint32_t N = (uint32_t)n;
    const bool flow = po && po->flow.rec;
    v.c = c; v.st = c->stream; v.vs = state_of(c);
    v.d_blob = d_blob; v.d_offsets = d_offsets; v.N = N; v.n_pi = n_pi; v.d_own_pi = d_own_pi;
    v.d_accept = d_accept; v.d_reason = d_reason; v.po = po;
    v.fargs = flow ? po->flow : FlowArgs{nullptr, nullptr, nullptr, 0};
    v.timing = c->opt.stage_times == 1;
    v.vs->clock.used = 0;
    v.vs->spans.clear();
    v.in = rsv::host::PlanInputs{N, v.co.n, v.co.cfg_of != nullptr, v.co.c[0][1], v.co.c[0][2], v.co.c[0][3], flow, po && po->paths(),
                                 po && po->d_sib, po && po->d_pair_sib, own, (size_t)MAX_FUSED};
    v.plan = rsv::host::plan_batch(c->opt, v.in);

    int rc = enqueue_inputs(v, pi);
    if (rc != RSV_OK) return rc;
    rc = enqueue_parse_transcript(v);
    if (rc != RSV_OK) return rc;
    rc = enqueue_slot_order(v);
    if (rc != RSV_OK) return rc;
    if (v.live) {
        rc = enqueue_row_hashes(v);
        if (rc != RSV_OK) return rc;
        rc = enqueue_query_stages(v);
        if (rc != RSV_OK) return rc;
    }
    return enqueue_finalize(v);
}

extern "C" {

int rsv_verify_batch_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                         const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint8_t* d_accept,
                         uint8_t* d_reason) {
    return nomem_guard([&] { return verify_impl(c, d_blob, d_offsets, n, cfg, pi, n_pi, nullptr, d_accept, d_reason, nullptr); });
}

int rsv_trace_paths_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                        const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint32_t n_queries, uint32_t max_log, uint32_t* d_sib,
                        uint32_t* d_pos, uint8_t* d_accept, uint8_t* d_reason) {
    if (!d_sib || !d_pos) return RSV_E_NULL;
    if (n_queries < 4 || n_queries > (uint32_t)MAXQ || max_log > (uint32_t)MAX_LOG) return RSV_E_SIZE;
    PathsOut po{d_sib, d_pos, n_queries, max_log, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, FlowArgs{}, nullptr, nullptr};
    return nomem_guard([&] { return verify_impl(c, d_blob, d_offsets, n, cfg, pi, n_pi, nullptr, d_accept, d_reason, &po); });
}

int rsv_fri_paths_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, const rsv_cfg_set* cfg, const rsv_public_input* pi,
                      size_t n_pi, uint32_t n_queries, uint32_t max_log, uint32_t n_inner, uint32_t* d_sib, uint32_t* d_cols,
                      uint8_t* d_accept, uint8_t* d_reason) {
    if (!d_sib || !d_cols) return RSV_E_NULL;
    if (n_queries < 4 || n_queries > (uint32_t)MAXQ || max_log > (uint32_t)MAX_LOG || n_inner > (uint32_t)MAX_INNER) return RSV_E_SIZE;
    PathsOut po{nullptr, nullptr, n_queries, max_log, d_sib, d_cols, n_inner, nullptr, nullptr, nullptr, nullptr, FlowArgs{}, nullptr, nullptr};
    return nomem_guard([&] { return verify_impl(c, d_blob, d_offsets, n, cfg, pi, n_pi, nullptr, d_accept, d_reason, &po); });
}

int rsv_verify_batch(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                     const rsv_public_input* pi, size_t n_pi, uint8_t* accept, uint8_t* reason, int device) {
    return nomem_guard([&]() -> int {
        if (n && (!blob || !offsets || !accept)) return RSV_E_NULL;
        if (n_pi && !pi) return RSV_E_NULL;
        { const int rc0 = check_cfg_set(cfg); if (rc0 != RSV_OK) return rc0; }  // (before any device work: misuse shows without a GPU)
        int rc = select_device(device);
        if (rc != RSV_OK) return rc;
        BatchStage b;
        rc = b.stage_cfg(cfg, n);
        if (rc != RSV_OK) return rc;
        if (n == 0) return RSV_OK;
        rc = b.open(blob, offsets, n, device);
        if (rc != RSV_OK) return rc;
        rc = rsv_verify_batch_dev(b.c(), b.d_blob, b.d_offsets, n, &b.cfg, pi, n_pi, b.d_accept, b.d_reason);
        return rc == RSV_OK ? b.finish(accept, reason) : rc;
    });
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
extern "C" {

int rsv_verify_hints_dev(rsv_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, const rsv_cfg_set* cfg, const rsv_public_input* pi,
                         size_t n_pi, const rsv_hints_out* out, uint8_t* d_accept, uint8_t* d_reason) {
    return nomem_guard([&] { return verify_hints_impl(c, d_blob, d_offsets, n, cfg, pi, n_pi, nullptr, out, d_accept, d_reason); });
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
    return nomem_guard([&]() -> int {
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
        BatchStage b;
        rc = b.stage_cfg(cfg, n);
        if (rc != RSV_OK) return rc;
        if (n == 0) return RSV_OK;
        rc = b.open(blob, offsets, n, device);
        if (rc != RSV_OK) return rc;
        const rsv_public_input* dpi = b.s.upload<rsv_public_input>(pi, sizeof(rsv_public_input) * n * n_pi, 16);
        if (b.s.rc != RSV_OK) return b.s.rc;
        rc = rsv_verify_batch_inputs_dev(b.c(), b.d_blob, b.d_offsets, n, &b.cfg, dpi, n_pi, b.d_accept, b.d_reason);
        return rc == RSV_OK ? b.finish(accept, reason) : rc;
    });
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
    return nomem_guard([&]() -> int {
        if (!out || (n && (!blob || !offsets || !accept))) return RSV_E_NULL;
        if (n_pi && !pi) return RSV_E_NULL;
        { const int rc0 = check_cfg_set(cfg); if (rc0 != RSV_OK) return rc0; }  // (before any device work: misuse shows without a GPU)
        if (n > (1u << 20)) return RSV_E_SIZE;
        int rc = select_device(device);
        if (rc != RSV_OK) return rc;
        BatchStage b;
        rc = b.stage_cfg(cfg, n);
        if (rc != RSV_OK) return rc;
        if (n == 0) return RSV_OK;
        rc = b.rebase(offsets, n);
        if (rc != RSV_OK) return rc;
        // the same struct, device side: one zero-filled allocation per requested output
        const size_t nq = out->n_queries, M = out->max_log, nt = 1 + (size_t)out->n_inner;
        rsv_hints_out dev = *out;
        bool shapeless = false;  // a requested output without a declared shape
        auto words = [&](uint32_t* host, size_t count) {
            if (host && count == 0) shapeless = true;
            return shapeless ? nullptr : b.s.output<uint32_t>(host, 4 * count, true);
        };
        if (out->d_flow_swap && out->flow_stride == 0) return RSV_E_SIZE;
        dev.d_accept_count = b.s.output<uint64_t>(out->d_accept_count, 8);
        dev.d_flow_swap = b.s.output<uint8_t>(out->d_flow_swap, n * (size_t)out->flow_stride, true);
        dev.d_transcript = words(out->d_transcript, n * (size_t)RSV_TRANSCRIPT_WORDS);
        dev.d_trace_sib = words(out->d_trace_sib, n * 4 * nq * M * 8);
        dev.d_trace_pos = words(out->d_trace_pos, n * 4 * nq);
        dev.d_trace_cols = words(out->d_trace_cols, n * 4 * nq * 64);
        dev.d_fri_sib = words(out->d_fri_sib, n * nt * nq * M * 8);
        dev.d_fri_cols = words(out->d_fri_cols, n * nt * nq * 3 * 8);
        dev.d_fri_folded = words(out->d_fri_folded, n * 3 * nq * 4);
        dev.d_query_values = words(out->d_query_values, n * nq * 4 * (8 + (size_t)out->n_inner));
        dev.d_flow = words(out->d_flow, n * (size_t)out->flow_stride * FLOW_WORDS);
        dev.d_flow_count = words(out->d_flow_count, n);
        dev.d_accept_bitmap = words(out->d_accept_bitmap, (n + 31) / 32);
        if (b.s.rc != RSV_OK) return b.s.rc;
        if (shapeless) return RSV_E_SIZE;
        rc = b.create(device);
        if (rc == RSV_OK) rc = b.upload(blob);
        if (rc != RSV_OK) return rc;
        rc = rsv_verify_hints_dev(b.c(), b.d_blob, b.d_offsets, n, &b.cfg, pi, n_pi, &dev, b.d_accept, b.d_reason);
        return rc == RSV_OK ? b.finish(accept, reason) : rc;
    });
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
    return nomem_guard([&]() -> int {
        if (n && !out) return RSV_E_NULL;
        std::vector<uint8_t> accept(n ? n : 1);
        rsv_hints_out ho{};
        ho.d_transcript = out;
        return rsv_verify_hints(blob, offsets, n, cfg, nullptr, 0, &ho, accept.data(), nullptr, device);
    });
}


// ---------------------------------------------------------------- a1 / a2 / a8 / line: arithmetic probes
int rsv_field_op(int op, const uint32_t* a4, const uint32_t* b4, uint32_t* out4, size_t n, int device) {
    return nomem_guard([&]() -> int {
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
        HostStage s;
        const uint32_t* da = s.upload<uint32_t>(a4, 16 * n);
        const uint32_t* db = binary ? s.upload<uint32_t>(b4, 16 * n) : nullptr;
        uint32_t* dout = s.output<uint32_t>(out4, 16 * n);
        if (s.rc != RSV_OK) return s.rc;
        hipLaunchKernelGGL(k_field_op, dim3(grid_for(n, 256)), dim3(256), 0, 0, op, da, db, dout, n);
        return s.finish();
    });
}

int rsv_domain_points(uint32_t log_size, const uint32_t* q, uint32_t* xy, size_t n, int device) {
    return nomem_guard([&]() -> int {
        if (n && (!q || !xy)) return RSV_E_NULL;
        if (log_size < 1 || log_size > (uint32_t)MAX_LOG || n > ((size_t)1 << 26)) return RSV_E_SIZE;
        int rc = select_device(device);
        if (rc != RSV_OK) return rc;
        if (n == 0) return RSV_OK;
        HostStage s;
        const uint32_t* dq = s.upload<uint32_t>(q, 4 * n);
        uint32_t* dxy = s.output<uint32_t>(xy, 8 * n);
        if (s.rc != RSV_OK) return s.rc;
        hipLaunchKernelGGL(k_domain_points, dim3(grid_for(n, 256)), dim3(256), 0, 0, log_size, dq, dxy, n);
        return s.finish();
    });
}

int rsv_line_eval(const uint32_t* coeffs4, uint32_t log_n, const uint32_t* x, uint32_t* out4, size_t n, int device) {
    return nomem_guard([&]() -> int {
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
        HostStage s;
        const uint32_t *dc = s.upload<uint32_t>(coeffs4, 16 * nc), *dx = s.upload<uint32_t>(x, 4 * n);
        uint32_t* dout = s.output<uint32_t>(out4, 16 * n);
        if (s.rc != RSV_OK) return s.rc;
        hipLaunchKernelGGL(k_line_eval, dim3(grid_for(n, 256)), dim3(256), 0, 0, dc, log_n, dx, dout, n);
        return s.finish();
    });
}

int rsv_last_layer_check(const uint32_t* coeffs4, uint32_t log_n, const uint32_t* x, const uint32_t* folded4, uint8_t* ok,
                         size_t n, int device) {
    return nomem_guard([&]() -> int {
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
        HostStage s;
        const uint32_t *dc = s.upload<uint32_t>(coeffs4, 16 * nc), *dx = s.upload<uint32_t>(x, 4 * n), *df = s.upload<uint32_t>(folded4, 16 * n);
        uint8_t* dok = s.output<uint8_t>(ok, n);
        if (s.rc != RSV_OK) return s.rc;
        hipLaunchKernelGGL(k_last_layer_check, dim3(grid_for(n, 256)), dim3(256), 0, 0, dc, log_n, dx, df, dok, n);
        return s.finish();
    });
}

// a10 probe: scatter the flattened samples to the word offsets the kernels read them from (a proof prefix per item)
int rsv_oods_eval(const uint32_t* samples4, const uint32_t* params26, uint32_t* out8, size_t n, int device) {
    return nomem_guard([&]() -> int {
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
        HostStage s;
        const uint32_t *dp = s.upload<uint32_t>(prefix.data(), 4 * prefix.size()), *dpar = s.upload<uint32_t>(params26, 4 * OODS_PARAM_WORDS * n);
        uint32_t* dout = s.output<uint32_t>(out8, 32 * n);
        if (s.rc != RSV_OK) return s.rc;
        launch_oods_probe(dp, (uint32_t)pw, dpar, dout, (uint32_t)n);
        return s.finish();
    });
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
    return nomem_guard([&]() -> int {
        if (!proof || !out) return RSV_E_NULL;
        if (cap < 1) return RSV_E_CAP;
        if (len > (1u << 30)) return RSV_E_SIZE;
        int rc = select_device(device);
        if (rc != RSV_OK) return rc;
        const uint64_t offs[2] = {0, len};
        std::vector<char> hm(sizeof(ProofMeta)), hc(sizeof(ProofCtx));
        HostStage s;
        const uint8_t* dblob = s.upload<uint8_t>(proof, len, BatchStage::kBlobSlack);
        const uint64_t* doffs = s.upload<uint64_t>(offs, 16);
        ProofMeta* dmeta = s.output<ProofMeta>(hm.data(), sizeof(ProofMeta));
        ProofCtx* dctx = s.output<ProofCtx>(hc.data(), sizeof(ProofCtx));
        uint32_t *dsum = s.scratch<uint32_t>(256, true), *dshape = s.scratch<uint32_t>(16);
        if (s.rc != RSV_OK) return s.rc;
        // probe: the configuration words serialized in the proof itself (documented in rsv.h: not a verdict)
        CfgSet co{};
        co.n = 1;
        if (len >= 4 * (W_NQ + 1)) {
            uint32_t hw[W_NQ + 1];
            memcpy(hw, proof, sizeof(hw));
            co.c[0][0] = hw[W_POW_BITS]; co.c[0][1] = hw[W_BLOWUP]; co.c[0][2] = hw[W_LOG_LAST]; co.c[0][3] = hw[W_NQ];
        }
        hipLaunchKernelGGL(k_parse, dim3(1), dim3(64), 0, 0, dblob, doffs, 1u, co, dmeta, dctx, dsum, dshape);
        // (the prefixes inside sampled_values are the OODS kernels' to check in the pipeline; no OODS evaluation runs here)
        hipLaunchKernelGGL(k_prefix_check, dim3(1), dim3(64), 0, 0, dblob, doffs, 1u, (const ProofMeta*)dmeta, dctx);
        {
            const bool row = default_options().transcript_form != 2;
            if (row)
                hipLaunchKernelGGL(k_transcript_row<0>, dim3(1), dim3(256), 0, 0, dblob, doffs, 1u, (const ProofMeta*)dmeta, dctx, FlowArgs{nullptr, nullptr, nullptr, 0});
            else
                hipLaunchKernelGGL(k_transcript<false>, dim3(1), dim3(64), 0, 0, dblob, doffs, 1u, (const ProofMeta*)dmeta, dctx, FlowArgs{nullptr, nullptr, nullptr, 0});
        }
        // no Merkle stage runs here: the whole proof is read for canonicity (k_finalize, force)
        hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, 0, dblob, doffs, 1u, (const ProofMeta*)dmeta, dctx, (uint8_t*)nullptr, (uint8_t*)nullptr, 1u,
                           (uint32_t*)nullptr, (unsigned long long*)nullptr);
        rc = s.finish();
        if (rc != RSV_OK) return rc;
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
    });
}

}  // extern "C"
