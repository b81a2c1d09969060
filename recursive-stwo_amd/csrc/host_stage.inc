// host_stage.inc — the one staging path of the host-pointer entry points (included by rsv_hip.hip ahead of every *_api.inc).
// HostStage: the device copies of one call's flat arguments, its 4-byte bad flag and the copy-back of its outputs — what a
// probe needs.  BatchStage, on top of it: a batch (blob, offsets) rebased to byte 0 and uploaded, the staged cfg_of, a
// context of the call's own with d_accept / d_reason — what rsv_verify_batch, _inputs, _hints and WitnessStage
// (witness_api.inc) need.  host_stream.inc and multi_api.inc keep their own pinned, pipelined staging.

namespace {

// RAII device buffer for the host-pointer convenience entry points.
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    // RSV_OPT_WS_FILL (process default): the fresh allocation holds the fill byte before anything is copied or launched into it
    hipError_t alloc(size_t bytes) {
        const size_t want = bytes ? bytes : 4;
        hipError_t e = hipMalloc(&p, want);
        const int fill = g_default_ws_fill.load(std::memory_order_relaxed);
        if (e == hipSuccess && fill) {
            e = hipMemset(p, fill - 1, want);
            if (e == hipSuccess) e = hipDeviceSynchronize();
        }
        return e;
    }
    template <class T> T* as() { return static_cast<T*>(p); }
};

int select_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return RSV_E_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return RSV_E_DEVICE;
    return RSV_OK;
}

// No exception leaves an extern "C" function: every entry point that stages host memory or reaches verify_impl (which keeps
// host vectors: buckets, groups) runs its body in here, and a std::bad_alloc is RSV_E_NOMEM.
template <class F> int nomem_guard(F f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return RSV_E_NOMEM;
    }
}

// The staged arguments of one call.  upload / output / scratch hand out device pointers and remember the first failure in
// `rc`, behind which every operation does nothing and returns NULL: a caller stages all its arguments, looks at rc once,
// launches, and calls finish().
struct HostStage {
    int rc = RSV_OK;

    // `bytes` of host memory on the device, `slack` spare bytes behind them; no host pointer, no device pointer
    template <class T> const T* upload(const void* host, size_t bytes, size_t slack = 0) {
        void* d = host ? fresh(bytes + slack) : nullptr;
        if (d && bytes) note(copy(d, host, bytes, hipMemcpyHostToDevice));
        return static_cast<const T*>(rc == RSV_OK ? d : nullptr);
    }
    // a device buffer that finish() copies back to `host`, in the order of registration; zero: it starts from zero
    template <class T> T* output(void* host, size_t bytes, bool zero = false) {
        void* d = host ? fresh(bytes) : nullptr;
        if (d && zero && bytes) note(zeroed(d, bytes));
        if (d) outs.push_back({host, d, bytes});
        return static_cast<T*>(rc == RSV_OK ? d : nullptr);
    }
    // a device buffer of the call that no host pointer stands behind
    template <class T> T* scratch(size_t bytes, bool zero = false) {
        void* d = fresh(bytes);
        if (d && zero && bytes) note(zeroed(d, bytes));
        return static_cast<T*>(rc == RSV_OK ? d : nullptr);
    }
    // the word a probe's kernel sets for a non-canonical input: zeroed here, read back by finish() ahead of the outputs
    uint32_t* bad_flag() { return flag = scratch<uint32_t>(4, true); }

    // Behind the launches (the null stream's, or streams the caller has synchronised): a set bad flag is RSV_E_RANGE with no
    // output written; else every output goes back.  Nothing is copied if anything before failed.
    int finish() {
        if (rc != RSV_OK) return rc;
        HIP_TRY(hipGetLastError());
        if (flag) {
            uint32_t bad = 0;
            HIP_TRY(hipMemcpy(&bad, flag, 4, hipMemcpyDeviceToHost));
            if (bad) return RSV_E_RANGE;
        }
        for (const Out& o : outs)
            if (o.bytes) HIP_TRY(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
        return RSV_OK;
    }

private:
    struct Out { void* host; void* dev; size_t bytes; };
    std::deque<DevBuf> bufs;
    std::vector<Out> outs;
    uint32_t* flag = nullptr;
    void note(int status) { if (rc == RSV_OK) rc = status; }
    void* fresh(size_t bytes) {
        if (rc != RSV_OK) return nullptr;
        bufs.emplace_back();
        note(allocate(bufs.back(), bytes));
        return rc == RSV_OK ? bufs.back().p : nullptr;
    }
    static int allocate(DevBuf& b, size_t bytes) { HIP_TRY(b.alloc(bytes)); return RSV_OK; }
    static int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { HIP_TRY(hipMemcpy(dst, src, bytes, kind)); return RSV_OK; }
    static int zeroed(void* d, size_t bytes) { HIP_TRY(hipMemset(d, 0, bytes)); return RSV_OK; }
};

// A batch in host memory on a context of the call's own.  The verify forms: stage_cfg() (the device is selected), then
// open(); WitnessStage takes the three steps of open() apart, its program upload between them.  Then the form's _dev call
// on c / d_blob / d_offsets / d_accept / d_reason (and &cfg), and finish().
struct BatchStage {
    HostStage s;  // every buffer of the call: the batch's own, and the outputs the form registers
    size_t n = 0;
    const uint8_t* d_blob = nullptr;
    const uint64_t* d_offsets = nullptr;
    uint8_t *d_accept = nullptr, *d_reason = nullptr;
    rsv_cfg_set cfg{};  // stage_cfg(): the caller's set, its cfg_of in device memory
    // The context is the LAST member, so it is destroyed FIRST, on every exit: rsv_ctx_destroy waits for the context's three
    // streams, and an error exit taken behind a launch may leave kernels in flight on them that still read and write the
    // buffers of `s` — those may be freed only behind that wait.
    struct Ctx {
        rsv_ctx* c = nullptr;
        ~Ctx() { rsv_ctx_destroy(c); }
    } ctx;
    rsv_ctx* c() const { return ctx.c; }

    // (the entry point has checked the set: check_cfg_set, ahead of select_device)
    int stage_cfg(const rsv_cfg_set* host, size_t n_proofs) {
        cfg = *host;
        cfg.cfg_of = n_proofs ? s.upload<uint8_t>(host->cfg_of, n_proofs) : nullptr;
        return s.rc;
    }
    // RSV_E_SIZE: the offsets decrease somewhere
    int rebase(const uint64_t* offsets, size_t n_proofs) {
        n = n_proofs;
        base = offsets[0];
        return rsv::host::rebase_offsets(offsets, n_proofs, rel);
    }
    int create(int device) { return rsv_ctx_create(device, &ctx.c); }
    // The blob from proof 0's first byte on, with kBlobSlack spare bytes behind the last proof (DESIGN.md §3: no kernel reads
    // past offsets[n], the slack is not relied on), the rebased offsets, and the two verdict arrays.
    int upload(const uint8_t* blob) {
        d_blob = s.upload<uint8_t>(blob + base, (size_t)rel[n], kBlobSlack);
        d_offsets = s.upload<uint64_t>(rel.data(), 8 * (n + 1));
        d_accept = s.scratch<uint8_t>(n);
        d_reason = s.scratch<uint8_t>(n);
        return s.rc;
    }
    int open(const uint8_t* blob, const uint64_t* offsets, size_t n_proofs, int device) {
        int rc = rebase(offsets, n_proofs);
        if (rc == RSV_OK) rc = create(device);
        return rc == RSV_OK ? upload(blob) : rc;
    }
    // Waits for the context (all three streams), then the registered outputs, accept and reason (may be NULL) go back.
    int finish(uint8_t* accept, uint8_t* reason) {
        int rc = s.rc != RSV_OK ? s.rc : rsv_ctx_synchronize(ctx.c);
        if (rc == RSV_OK) rc = s.finish();
        if (rc != RSV_OK) return rc;
        HIP_TRY(hipMemcpy(accept, d_accept, n, hipMemcpyDeviceToHost));
        if (reason) HIP_TRY(hipMemcpy(reason, d_reason, n, hipMemcpyDeviceToHost));
        return RSV_OK;
    }

    static constexpr size_t kBlobSlack = 16;

private:
    uint64_t base = 0;
    std::vector<uint64_t> rel;
};

}  // namespace
