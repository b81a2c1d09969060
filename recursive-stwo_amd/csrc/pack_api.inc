// pack_api.inc — rsv_proof_bytes and rsv_proof_pack_dev (the next proof serialised on the device into the verifier's blob
// layout): k_pack.hpp, include/rsv.h.  Included at the end of rsv_hip.hip, after fri_open_api.inc.
//
// The map of the prefixes (k_pack.hpp) depends on the configuration words and T only, so the context keeps the one of its
// last call: the first call of a configuration builds it on the host and uploads it, every later one enqueues three kernels.

namespace {

constexpr size_t PK_MAX_ROWS = 65535;  // grid rows of one launch (gridDim.y)

// Context state of the serialiser: the map of the last configuration (host copy and device copy) and the workspace.
struct PackState {
    uint32_t key[7] = {};
    bool valid = false;
    std::vector<uint2> map;
    std::vector<uint32_t> pre_at;
    void* d_map = nullptr;
    size_t d_map_bytes = 0;
    void* ws = nullptr;  // begin tables and lengths of a call
    size_t ws_bytes = 0;
};
void destroy_pack_state(PackState* s) {
    if (s->d_map) (void)hipFree(s->d_map);
    if (s->ws) (void)hipFree(s->ws);
    delete s;
}

// The map and pre_at [R + 1] of key = (log_size_plonk, log_size_poseidon, pow_bits, log_blowup, log_last, n_queries, T):
// chain.proof_bytes field by field, the copies left out.
void pk_build(const uint32_t* key, std::vector<uint2>& map, std::vector<uint32_t>& pre_at) {
    const uint32_t T = key[6], log_last = key[4];
    map.clear();
    pre_at.clear();
    const auto lit = [&](uint32_t v) { map.push_back(make_uint2(rsv::PK_LIT, v)); };
    const auto u64 = [&](uint64_t v) { lit((uint32_t)v); lit((uint32_t)(v >> 32)); };
    const auto src = [&](uint32_t part, uint32_t at, uint32_t words) {
        for (uint32_t i = 0; i < words; i++) map.push_back(make_uint2(rsv::PK_SRC + part, at + i));
    };
    const auto run = [&]() { pre_at.push_back((uint32_t)map.size()); };
    const auto count = [&]() { map.push_back(make_uint2(rsv::PK_CNT, (uint32_t)pre_at.size() - 1)); lit(0); };
    run();  // 0: the head, then the decommitments
    lit(key[0]);
    lit(key[1]);
    src(rsv::PK_SUMS, 0, 8);
    lit(key[2]);
    lit(key[3]);
    lit(key[4]);
    u64(key[5]);
    u64(4);
    src(rsv::PK_ROOTS, 0, 24);
    src(rsv::PK_ROOT3, 0, 8);
    u64(4);
    static const uint32_t columns[4] = {50, 60, 16, 8};
    uint32_t at = 0;
    for (uint32_t t = 0; t < 4; t++) {
        u64(columns[t]);
        if (t == 3) at = 0;
        for (uint32_t c = 0; c < columns[t]; c++) {
            const uint32_t k = t == 2 && (c & 4) ? 2 : 1;  // tree 2: 1, 1, 1, 1, 2, 2, 2, 2 twice
            u64(k);
            src(t == 3 ? rsv::PK_SAMPLES3 : rsv::PK_SAMPLES, at, 4 * k);
            at += 4 * k;
        }
    }
    u64(4);
    count();
    for (uint32_t t = 1; t < 4; t++) {
        run();
        u64(0);
        count();
    }
    run();  // 4: the queried values
    u64(0);
    u64(4);
    count();
    for (uint32_t t = 1; t < 4; t++) {
        run();
        count();
    }
    for (uint32_t t = 0; t < T; t++) {
        run();
        if (t == 0) {
            src(rsv::PK_NONCE, 0, 2);
        } else {
            u64(0);
            src(rsv::PK_FRI_ROOTS, 8 * (t - 1), 8);
            if (t == 1) u64(T - 1);
        }
        count();
        run();
        count();
    }
    run();  // the last polynomial
    u64(0);
    src(rsv::PK_FRI_ROOTS, 8 * (T - 1), 8);
    if (T == 1) u64(0);
    u64((uint64_t)1 << log_last);
    run();
    lit(log_last);
    run();
}

// Words of a proof with the given counts (values 0-3, witness nodes 0-3, then per layer tree fri_witness values and
// hash_witness nodes): the prefixes, the copies, the last polynomial.
uint64_t pk_words(uint32_t log_last, uint32_t T, const uint64_t* counts) {
    const uint32_t key[7] = {0, 0, 0, 0, log_last, 0, T};
    std::vector<uint2> map;
    std::vector<uint32_t> pre_at;
    pk_build(key, map, pre_at);
    uint64_t words = map.size() + ((uint64_t)4 << log_last);
    for (uint32_t t = 0; t < 4; t++) words += counts[t] + 8 * counts[4 + t];
    for (uint32_t t = 0; t < T; t++) words += 4 * counts[8 + 2 * t] + 8 * counts[9 + 2 * t];
    return words;
}

bool pk_list_null(const rsv_proof_list& l) { return !l.d_items || !l.d_count; }
bool pk_list_odd(const rsv_proof_list& l) { return ((uintptr_t)l.d_items & 3) || ((uintptr_t)l.d_count & 3); }
rsv::PkList pk_list(const rsv_proof_list& l) { return rsv::PkList{l.d_items, l.stride, l.d_count, l.count_stride, l.cap}; }

}  // namespace

extern "C" {

int rsv_proof_bytes(uint32_t log_last, uint32_t n_layers, const uint32_t* counts, size_t* bytes) {
    if (!counts || !bytes) return RSV_E_NULL;
    if (log_last > RSV_MAX_LOG_LAST_LAYER || n_layers < 1 || n_layers > rsv::PK_MAX_T) return RSV_E_SIZE;
    uint64_t c[8 + 2 * rsv::PK_MAX_T];
    for (uint32_t i = 0; i < 8 + 2 * n_layers; i++) c[i] = counts[i];
    *bytes = (size_t)(4 * pk_words(log_last, n_layers, c));
    return RSV_OK;
}

int rsv_proof_pack_dev(rsv_ctx* c, const rsv_proof_parts* parts, size_t n, const uint8_t* d_mask, uint8_t* d_blob, size_t blob_cap,
                       uint64_t* d_offsets) {
    static_assert(rsv::PK_MAX_T == 1 + RSV_MAX_FRI_INNER, "include/rsv.h");
    if (!c || !parts || !d_offsets) return RSV_E_NULL;
    const rsv_proof_parts& q = *parts;
    if (!q.d_sums || !q.d_roots || !q.d_root3 || !q.d_samples || !q.d_samples3 || !q.d_nonce || !q.d_fri_roots || !q.d_last_poly) return RSV_E_NULL;
    for (int t = 0; t < 4; t++)
        if (pk_list_null(q.values[t]) || pk_list_null(q.witness[t])) return RSV_E_NULL;
    if (pk_list_null(q.fri_witness) || pk_list_null(q.fri_hash_witness)) return RSV_E_NULL;
    if (n == 0 || n > (1u << 20)) return RSV_E_SIZE;
    const rsv_pcs_config cfg{q.pow_bits, q.log_blowup, q.log_last, q.n_queries};
    if (rsv_cfg_check(&cfg) != RSV_OK) return RSV_E_SIZE;
    const uint32_t T = q.n_layers;
    if (T < 1 || T > rsv::PK_MAX_T) return RSV_E_SIZE;
    if (((uintptr_t)q.d_sums & 3) || ((uintptr_t)q.d_roots & 3) || ((uintptr_t)q.d_root3 & 3) || ((uintptr_t)q.d_samples & 3) ||
        ((uintptr_t)q.d_samples3 & 3) || ((uintptr_t)q.d_nonce & 3) || ((uintptr_t)q.d_fri_roots & 3) || ((uintptr_t)q.d_last_poly & 3) ||
        ((uintptr_t)d_blob & 3) || ((uintptr_t)d_offsets & 7) || pk_list_odd(q.fri_witness) || pk_list_odd(q.fri_hash_witness))
        return RSV_E_SIZE;
    uint64_t caps[8 + 2 * rsv::PK_MAX_T];
    for (int t = 0; t < 4; t++) {
        const rsv_proof_list &v = q.values[t], &w = q.witness[t];
        if (pk_list_odd(v) || pk_list_odd(w)) return RSV_E_SIZE;
        if (v.stride < v.cap || w.stride < (uint64_t)w.cap * 8) return RSV_E_SIZE;
        caps[t] = v.cap;
        caps[4 + t] = w.cap;
    }
    if (q.fri_witness.stride < (uint64_t)T * q.fri_witness.cap * 4 || q.fri_hash_witness.stride < (uint64_t)T * q.fri_hash_witness.cap * 8 ||
        q.fri_witness.count_stride < T || q.fri_hash_witness.count_stride < T)
        return RSV_E_SIZE;
    for (uint32_t t = 0; t < T; t++) {
        caps[8 + 2 * t] = q.fri_witness.cap;
        caps[9 + 2 * t] = q.fri_hash_witness.cap;
    }
    // the kernels count a proof's words in 32 bits, its bytes too
    const uint64_t max_words = pk_words(q.log_last, T, caps);
    if (max_words > ((uint64_t)1 << 30)) return RSV_E_SIZE;

    HIP_TRY(hipSetDevice(c->device));
    if (!c->pack) c->pack = new (std::nothrow) PackState();
    if (!c->pack) return RSV_E_NOMEM;
    PackState& s = *c->pack;
    hipStream_t st = c->stream;
    const uint32_t R = rsv::pk_runs(T);
    const uint32_t key[7] = {q.log_size_plonk, q.log_size_poseidon, q.pow_bits, q.log_blowup, q.log_last, q.n_queries, T};
    if (!s.valid || memcmp(key, s.key, sizeof key) != 0) {
        // the copy before may still be read from the host vectors: wait for it before they change
        if (s.valid) HIP_TRY(hipStreamSynchronize(st));
        s.valid = false;
        pk_build(key, s.map, s.pre_at);
        const size_t map_bytes = s.map.size() * sizeof(uint2);
        const int rc = ensure_buf(c, &s.d_map, &s.d_map_bytes, map_bytes + s.pre_at.size() * sizeof(uint32_t));
        if (rc != RSV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(s.d_map, s.map.data(), map_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(s.d_map) + map_bytes, s.pre_at.data(), s.pre_at.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        memcpy(s.key, key, sizeof key);
        s.valid = true;
    }
    const size_t len_bytes = n * sizeof(uint64_t);
    const int rc = ensure_buf(c, &s.ws, &s.ws_bytes, len_bytes + n * (R + 1) * sizeof(uint32_t));
    if (rc != RSV_OK) return rc;

    rsv::PkArgs a{};
    for (int t = 0; t < 4; t++) {
        a.witness[t] = pk_list(q.witness[t]);
        a.values[t] = pk_list(q.values[t]);
    }
    a.fri_witness = pk_list(q.fri_witness);
    a.fri_hash_witness = pk_list(q.fri_hash_witness);
    a.sums = q.d_sums;
    a.roots = q.d_roots;
    a.root3 = q.d_root3;
    a.samples = q.d_samples;
    a.samples3 = q.d_samples3;
    a.nonce = q.d_nonce;
    a.fri_roots = q.d_fri_roots;
    a.last_poly = q.d_last_poly;
    a.mask = d_mask;
    a.map = static_cast<const uint2*>(s.d_map);
    a.pre_at = reinterpret_cast<const uint32_t*>(a.map + s.map.size());
    a.len = static_cast<uint64_t*>(s.ws);
    a.begin = reinterpret_cast<uint32_t*>(static_cast<char*>(s.ws) + len_bytes);
    a.T = T;
    a.log_last = q.log_last;
    hipLaunchKernelGGL(rsv::k_pk_sizes, dim3((unsigned)n), dim3(64), 0, st, a);
    hipLaunchKernelGGL(rsv::k_pk_scan, dim3(1), dim3(n <= 64 ? 64 : rsv::PK_SCAN), 0, st, a.len, (uint32_t)n, d_offsets);
    if (d_blob) {
        const unsigned blocks = grid_for(max_words, 256);
        for (size_t p0 = 0; p0 < n; p0 += PK_MAX_ROWS) {
            const size_t rows = std::min(PK_MAX_ROWS, n - p0);
            hipLaunchKernelGGL(rsv::k_pk_pack, dim3(blocks, (unsigned)rows), dim3(256), 0, st, a, (uint32_t)p0, d_offsets,
                               reinterpret_cast<uint32_t*>(d_blob), (uint64_t)blob_cap);
        }
    }
    HIP_TRY(hipGetLastError());
    return RSV_OK;
}

}  // extern "C"
