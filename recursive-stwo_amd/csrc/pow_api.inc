// pow_api.inc — rsv_pow_grind_dev (the search for the proof-of-work nonce, its mix into the channel) and
// rsv_draw_queries_dev (the query positions): k_pow.hpp, include/rsv.h.  Included at the end of rsv_hip.hip, after
// fri_api.inc.

namespace {

constexpr size_t POW_MAX_ROWS = 65535;  // grid rows of one launch (gridDim.y)

// Workgroups per proof of a search launch over `rows` proofs (k_pow.hpp, GRID): min(2^pow_bits, max_tries) lanes in whole
// workgroups, at most the machine's 8 resident workgroups per CU shared among the rows, at least one.
unsigned pow_row_blocks(const rsv_ctx* c, uint32_t pow_bits, uint64_t max_tries, size_t rows) {
    const uint64_t lanes = std::min<uint64_t>((uint64_t)1 << pow_bits, max_tries);
    const uint64_t want = (lanes + rsv::POW_BLOCK - 1) / rsv::POW_BLOCK;
    const uint64_t fill = std::max<uint64_t>((uint64_t)c->n_cu * 8 / rows, 1);
    return (unsigned)std::max<uint64_t>(std::min(want, fill), 1);
}

}  // namespace

extern "C" {

int rsv_pow_grind_dev(rsv_ctx* c, uint32_t pow_bits, uint64_t start, uint64_t max_tries, size_t n, uint8_t* d_ok, uint32_t* d_channel,
                      uint32_t* d_nonce) {
    if (!c || !d_ok || !d_channel || !d_nonce) return RSV_E_NULL;
    if (pow_bits > RSV_MAX_POW_BITS || n == 0 || n > (1u << 20)) return RSV_E_SIZE;
    if (max_tries == 0) max_tries = (uint64_t)1 << (pow_bits + 6);
    if (start + max_tries < start) return RSV_E_SIZE;  // every candidate is below 2^64 - 1
    if (((uintptr_t)d_channel & 3) || ((uintptr_t)d_nonce & 3)) return RSV_E_SIZE;
    HIP_TRY(hipSetDevice(c->device));
    const int rc = ensure_buf(c, &c->ws_pow, &c->ws_pow_bytes, n * sizeof(unsigned long long));
    if (rc != RSV_OK) return rc;
    unsigned long long* best = static_cast<unsigned long long*>(c->ws_pow);
    hipStream_t st = c->stream;
    HIP_TRY(hipMemsetAsync(best, 0xff, n * sizeof(unsigned long long), st));
    for (size_t p0 = 0; p0 < n; p0 += POW_MAX_ROWS) {
        const size_t rows = std::min(POW_MAX_ROWS, n - p0);
        hipLaunchKernelGGL(rsv::k_pow_search, dim3(pow_row_blocks(c, pow_bits, max_tries, rows), (unsigned)rows), dim3(rsv::POW_BLOCK), 0, st,
                           d_channel, d_ok, (uint32_t)p0, pow_bits, start, max_tries, best);
    }
    hipLaunchKernelGGL(rsv::k_pow_finish, dim3(grid_for(n, 64)), dim3(64), 0, st, best, (uint32_t)n, d_ok, d_channel, d_nonce);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

int rsv_draw_queries_dev(rsv_ctx* c, size_t n, const uint8_t* d_mask, uint32_t n_queries, uint32_t log_size, uint32_t log_size_low,
                         uint32_t* d_channel, uint32_t* d_queries, uint32_t* d_queries_low) {
    if (!c || !d_channel || !d_queries) return RSV_E_NULL;
    if (n == 0 || n > (1u << 20) || n_queries < 1 || n_queries > RSV_MAX_QUERIES) return RSV_E_SIZE;
    if (log_size_low < 1 || log_size_low > log_size || log_size > RSV_MAX_LOG_SIZE) return RSV_E_SIZE;
    if (((uintptr_t)d_channel & 3) || ((uintptr_t)d_queries & 3) || ((uintptr_t)d_queries_low & 3)) return RSV_E_SIZE;
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(rsv::k_pow_queries, dim3(grid_for(n, 64)), dim3(64), 0, c->stream, d_mask, (uint32_t)n, n_queries, log_size, log_size_low,
                       d_channel, d_queries, d_queries_low);
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

}  // extern "C"
