/*
 * rsv.h — C-ABI drop-in boundary of the MI355X-native batch verifier for
 * Poseidon31-channel "Plonk-with-Poseidon" Circle-STARK proofs.
 *
 * The reference (Bitcoin-Wildlife-Sanctuary/recursive-stwo) has no FFI of its
 * own: the verify path is reached through Rust generics.  Every entry point
 * below names the reference item whose *values* it replaces (paths relative to
 * the reference root); INTEGRATION.md shows the Rust `extern "C"` block a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - All field elements are canonical M31 words (0 <= w < 2^31-1) in
 *     little-endian u32.  QM31 = 4 words (a0,a1,b0,b1) for (a0+a1*i)+(b0+b1*i)*u.
 *     A hash is 8 words.
 *   - Return value: RSV_OK (0) on success, negative rsv_status on API misuse
 *     or device failure.  A proof that does not verify is DATA
 *     (accept[i]=0, reason[i]=why), never an error and never an abort.
 *   - The caller owns every buffer.  Functions taking `device` copy host
 *     buffers to that HIP device and back (stream-ordered, synchronous on
 *     return).  `_dev` variants take device pointers already resident in HBM
 *     and enqueue on the context's stream.
 *   - There is NO CPU fallback in this library: if no HIP device is usable the
 *     call fails with RSV_E_DEVICE.
 *   - Thread-safety: distinct rsv_ctx objects may be used concurrently; one
 *     ctx is single-threaded (mirrors the `!Send` reference types,
 *     constraint_system/src/lib.rs:33).
 */
#ifndef RSV_H_
#define RSV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSV_M31_P 0x7fffffffu
#define RSV_ABI_VERSION 6

typedef enum rsv_status {
    RSV_OK = 0,
    RSV_E_NULL = -1,     /* required pointer is NULL */
    RSV_E_SIZE = -2,     /* inconsistent sizes / offsets not monotone / n too large */
    RSV_E_DEVICE = -3,   /* no such HIP device, or a HIP call failed */
    RSV_E_CAP = -4,      /* output capacity too small */
    RSV_E_RANGE = -5,    /* input word not a canonical M31 */
    RSV_E_UNAVAILABLE = -6, /* an optional run-time dependency (RCCL, for rsv_exchange_*) could not be loaded */
    RSV_E_NOMEM = -7     /* host memory for the call's staging could not be allocated (no verdict was written) */
} rsv_status;

/* Why proof i was rejected.  Order = the order in which the reference's
 * stages would panic (examples/single-proof/src/main.rs:33-82).
 *
 * Reason codes are this library's extension: the reference panics at the first failed check, so only accept / reject
 * is pinned by its fixtures; which code a rejected proof gets is defined here and checked against this repo's oracle.
 *
 * KNOWN DIVERGENCE from "bit-exact accept / reject on identical bytes" (deliberate, on the safe side): every
 * field-element word of a proof must be canonical (< 2^31-1), otherwise the proof is RSV_R_PARSE.  bincode
 * deserialises M31(u32) unchecked and stwo's release-mode arithmetic reduces such a word (partial_reduce maps P to
 * 0), so the Rust verifier most likely ACCEPTS a genuine proof in which a 0 word has been re-encoded as P
 * (0x7fffffff), and panics on overflow in debug builds for larger words; this library rejects all of them.  No
 * reference fixture contains such a word, and without a Rust toolchain the reference's behaviour on one cannot be
 * observed here.  Exempt (not field elements, read by nothing else): the two halves of the 64-bit proof-of-work
 * nonce and the proof's final word, last_layer_poly.log_size. */
typedef enum rsv_reason {
    RSV_R_OK = 0,
    RSV_R_PARSE = 1,        /* bincode shape / config mismatch (examples/single-proof/src/main.rs:24-31), a non-canonical field
                               element, or a header beyond this library's shape limits (RSV_MAX_*, below) */
    RSV_R_POW = 2,          /* components/recursive/fiat_shamir/src/lib.rs:115-117 */
    RSV_R_LOGUP = 3,        /* components/recursive/fiat_shamir/src/lib.rs:133-141 */
    RSV_R_COMPOSITION = 4,  /* components/recursive/composition/src/lib.rs:106-120 */
    RSV_R_DUP_QUERY = 5,    /* components/recursive/answer/src/lib.rs:190-195 */
    RSV_R_MERKLE_T0 = 6,    /* components/recursive/answer/src/lib.rs:214-258 (tree 0..3) */
    RSV_R_MERKLE_T1 = 7,
    RSV_R_MERKLE_T2 = 8,
    RSV_R_MERKLE_T3 = 9,
    RSV_R_FRI_FIRST = 10,   /* components/recursive/folding/src/lib.rs:23-54 */
    RSV_R_FRI_INNER = 11,   /* components/recursive/folding/src/lib.rs:135-192 */
    RSV_R_FRI_LAST = 12     /* components/recursive/folding/src/lib.rs:194-204 */
} rsv_reason;

/* stwo PcsConfig{pow_bits, FriConfig::new(log_last_layer_degree_bound,
 * log_blowup_factor, n_queries)} as written in
 * examples/multi-proofs/src/main.rs:173-196. */
typedef struct rsv_pcs_config {
    uint32_t pow_bits;
    uint32_t log_blowup_factor;
    uint32_t log_last_layer_degree_bound;
    uint32_t n_queries;
} rsv_pcs_config;

/* SHAPE LIMITS of this library (the reference has none: its vectors grow with the proof).  Tables in HBM and LDS are
 * sized by them.
 *   A CONFIGURATION beyond them is refused: every entry point that takes an rsv_cfg_set returns RSV_E_SIZE (and writes
 *   no verdict) unless every configuration of the set has
 *       1 <= n_queries <= RSV_MAX_QUERIES,  1 <= log_blowup_factor <= RSV_MAX_LOG_BLOWUP,
 *       log_last_layer_degree_bound <= RSV_MAX_LOG_LAST_LAYER,  pow_bits <= RSV_MAX_POW_BITS;
 *   rsv_cfg_check tells without a device.
 *   A PROOF whose own header goes beyond them — component log sizes (log_size_plonk, log_size_poseidon) outside
 *   1 .. RSV_MAX_COMPONENT_LOG, or a largest column log size M = max(log_size_plonk + 1, log_size_poseidon + 2) +
 *   log_blowup_factor above RSV_MAX_LOG_SIZE (which also bounds the FRI inner layers by RSV_MAX_FRI_INNER) — is data, not
 *   misuse: it is rejected with RSV_R_PARSE like any proof this library cannot read, although the reference would verify
 *   it if it is genuine.  (Every fixture of the reference: n_queries 8 .. 80, M 21 .. 28, 7 .. 12 inner layers.)
 *   The witness entry points (rsv_witness_*) additionally need log_size_plonk, log_size_poseidon <= RSV_MAX_WITNESS_LOG. */
#define RSV_MAX_QUERIES 128
#define RSV_MAX_LOG_BLOWUP 16
#define RSV_MAX_LOG_LAST_LAYER 16
#define RSV_MAX_POW_BITS 30
#define RSV_MAX_COMPONENT_LOG 28
#define RSV_MAX_LOG_SIZE 30
#define RSV_MAX_FRI_INNER 28
#define RSV_MAX_WITNESS_LOG 24
/* RSV_OK if the library can verify proofs under *cfg, RSV_E_SIZE if it is beyond the limits above, RSV_E_NULL. */
int rsv_cfg_check(const rsv_pcs_config* cfg);

/* The configuration(s) the caller expects — REQUIRED by every entry point that produces a verdict.  The reference
 * never takes the configuration from the proof: FiatShamirHints::new(&proof, config, ..)
 * (components/hints/src/fiat_shamir.rs:69-74), examples/multi-proofs/src/main.rs:173-196 pass it in; a verifier that
 * trusted the serialized words would let a forger choose pow_bits = 0, n_queries = 1.  Proof i must carry exactly
 * cfgs[cfg_of ? cfg_of[i] : 0] in its header, else it is rejected with RSV_R_PARSE.
 *   cfgs    n_cfgs (1..RSV_MAX_CFGS) configurations, HOST memory
 *   cfg_of  one index per proof (a mixed batch, e.g. the 6 configurations of the multi-proofs chain) or NULL;
 *           same residency as the blob: device memory for the _dev entry points, host memory otherwise.
 *           An index >= n_cfgs rejects the proof (RSV_R_PARSE). */
#define RSV_MAX_CFGS 16
typedef struct rsv_cfg_set {
    const rsv_pcs_config* cfgs;
    uint32_t n_cfgs;
    const uint8_t* cfg_of;
} rsv_cfg_set;

/* One public input `(wire index, QM31 value)` as passed to
 * FiatShamirResults::compute(.., inputs) (components/recursive/fiat_shamir/src/lib.rs:31-36). */
typedef struct rsv_public_input {
    uint32_t idx;
    uint32_t value[4];
} rsv_public_input;

/* Opaque per-device context: HIP stream + reusable HBM workspace. */
typedef struct rsv_ctx rsv_ctx;

int rsv_abi_version(void);
/* Number of usable HIP devices (0 if none; never fails). */
int rsv_device_count(void);
int rsv_ctx_create(int device, rsv_ctx** out);
void rsv_ctx_destroy(rsv_ctx* ctx);
/* Block until everything enqueued on the context's stream has finished. */
int rsv_ctx_synchronize(rsv_ctx* ctx);
/* The context's hipStream_t (as void*), so a caller can order its own work. */
void* rsv_ctx_stream(rsv_ctx* ctx);
/* Stream ordering with the caller's own HIP work (the context enqueues on private non-blocking streams):
 *   rsv_ctx_wait_stream   everything enqueued so far on `hip_stream` (a hipStream_t; NULL = the legacy default stream)
 *                         happens before whatever is enqueued on the context next — call it after producing the
 *                         blob / offsets / output buffers with your own kernels or copies, before a _dev entry point;
 *   rsv_stream_wait_ctx   the reverse: `hip_stream` waits for everything the context has enqueued so far.
 * Neither blocks the host. */
int rsv_ctx_wait_stream(rsv_ctx* ctx, void* hip_stream);
int rsv_stream_wait_ctx(rsv_ctx* ctx, void* hip_stream);

/* Tuning / diagnostic knobs.  The library never reads the environment: a knob changes only through this call, on one
 * context, or — ctx == NULL — as the process default that contexts created LATER inherit (the host-pointer
 * convenience entry points create a context of their own, so that is how the tests steer them).  Every knob only
 * selects between kernel forms / launch layouts that give bit-identical verdicts (the parity tests run each of them
 * against the oracle); 0 is always "automatic" (= what production runs).  Returns RSV_E_SIZE for an unknown option,
 * RSV_E_RANGE for a value outside the listed range. */
typedef enum rsv_option {
    RSV_OPT_TRANSCRIPT_FORM = 1,  /* 0 auto (by batch size), 1 one proof per 16-lane DPP row, 2 one proof per lane */
    RSV_OPT_TRANSCRIPT_SPLIT = 2, /* row form only: 0 auto, 1 one launch, 2 front half beside the parser + back half; a lane-form
                                     batch runs its transcript as one launch whatever this says */
    RSV_OPT_OODS_FORM = 3,        /* 0 auto, 1 row, 2 lane */
    RSV_OPT_QCONST_FORM = 4,      /* 0 auto (<= 4 096 proofs: four 16-lane rows per proof, <= 24 576: one row, else lane), 1 one row per proof, 2 lane */
    RSV_OPT_PLAN_FORM = 5,        /* 0 / 1 one lane per (proof, query), 2 one lane per proof */
    RSV_OPT_TREE_CAP = 6,         /* 0 / 1 dense top-of-tree cap, 2 every lane walks its path to the root */
    RSV_OPT_OVERLAP_TREES = 7,    /* 0 auto, 1 FRI trees beside the trace trees (single-group batches), 2 behind them */
    RSV_OPT_WS_BUDGET_MB = 8,     /* 1 .. 2^20: budget of the per-query workspace (default 8192); larger batches are cut into groups */
    RSV_OPT_PERM_WG_PER_CU = 9,   /* 1 .. 32: workgroups per CU of the grid-stride rsv_poseidon2_permute kernel (default 24) */
    RSV_OPT_HOST_CHUNK_MB = 10,   /* 1 .. 16384: staging chunk of rsv_verify_batch_host (default 256) */
    RSV_OPT_HOST_THREADS = 11,    /* 0 = min(cores, 4), else 1 .. 64 gather threads of rsv_verify_batch_host */
    RSV_OPT_DEBUG_LOG = 12,       /* 0 / 1: print failing HIP calls to stderr (process-wide, ctx ignored) */
    RSV_OPT_CRITICAL_CHAIN = 13,  /* 0 auto, 1 the step's chain of dependent kernels on one stream, 2 the two-stream layout */
    RSV_OPT_DEVICE_ORDER = 14,    /* 0 / 1 batches under one configuration: slot order by shape on the device, no host round
                                     trip inside the call; 2 the host-side bucketing of multi-configuration batches */
    RSV_OPT_WITNESS_LAYOUT = 16,  /* rsv_witness_eval_dev's d_variables: 0 / 1 [proof][variable] (the reference's vector per
                                     proof); 2 [variable][proof] — what the level kernels write: no transpose (a third of
                                     the traffic) and no second copy in scratch, for consumers that gather for many proofs */
    RSV_OPT_WITNESS_SMALL_MAX = 17, /* rsv_witness_eval_dev: 0 default (by batch and program size), else 1 + the largest batch whose
                                     program runs in ONE launch (a workgroup per few proofs walks all levels) instead of one
                                     launch per level; 1 = never */
    RSV_OPT_WITNESS_SMALL_LOG = 18, /* 0 default, else 1 + log2(proofs per workgroup) of that form, 1 .. 7 */
    RSV_OPT_WITNESS_WALK_LOG = 20, /* rsv_witness_eval_dev, batches that run the program level by level: the levels behind the
                                     program's wide head in ONE launch, a workgroup per 2^k proofs: 0 auto, 1 off, else 1 + k (k = 1 .. 6) */
    RSV_OPT_FLOW_CAP = 21,        /* passes that emit the PoseidonFlow: 0 / 1 a node several queries share is hashed once and the record
                                     of every query through it written from there, 2 every lane hashes its whole path itself */
    RSV_OPT_PAIR_ORDER = 22,      /* 0 / 1 a k_pair_merkle launch that is resident all at once deals its FRI trees (grid rows) out over the
                                     compute units by depth (the dispatcher does not balance such a launch), 2 grid row y = tree y */
    RSV_OPT_TREE_PACE = 23,       /* 0 auto (small batches: 2, a few hundred proofs and fewer: 3), 1 the Merkle kernels call the permutation
                                     instance with wait states behind its multiplies (pays with several waves per SIMD), 2 the one
                                     without (a wave nearly alone), 3 the row form: 16 threads per Merkle path share every permutation
                                     (a launch of a few waves: the walk is a chain of dependent permutations, the row form's a
                                     quarter as long); not with more than 32 queries (then: 2, or 1 when the flow is written) */
    RSV_OPT_QUERY_FORM = 25,      /* 0 auto (by batch size), 1 the quotient / fold kernel with a row of 16 threads per query that split its sums
                                     (chain layout only; not with more than 32 queries), 2 with one lane per query */
    RSV_OPT_STAGE_TIMES = 24,     /* 0 / 2 off; 1 record a HIP event pair around every stage of a verify call, which is what
                                     rsv_last_stage_times reads.  Off by default: the records cost ~8 us of queue time per stage */
    RSV_OPT_CAP_MID = 26,         /* with the cap's top in kernels of its own (RSV_OPT_CAP_TOP): 0 auto — a bucket of proofs whose dense cap levels
                                     fill the tree kernels' waves badly (80, 27, 11, 10 queries) hands its nodes over at the cap level, a
                                     lane per subtree walks the middle levels (k_cap_mid), k_cap_top the rest; 1 every bucket does, 2 none */
    RSV_OPT_CIRCUIT_EVAL_FORM = 30, /* rsv_circuit_eval_dev: 0 auto (by batch size), 1 one launch per level of the evaluation program, 2 one
                                     launch in which a workgroup per witness walks the levels */
    RSV_OPT_STATEMENT_ROW_MAX = 31, /* rsv_statement_digest_dev: 0 default (24 576, measured), else 1 + the largest number of groups hashed in the
                                     row form (16 threads per group share every permutation: a group's permutations depend on
                                     one another); more groups take one lane each; 1 = never the row form, 0 .. 2^26 + 1 */
    RSV_OPT_WS_FILL = 32,         /* DIAGNOSTIC, the one knob that is no choice between kernel forms.  0 off: exactly the code path without
                                     it.  v = 1 .. 256: every byte of the library's own device scratch holds v - 1 before the first
                                     kernel of a call can touch it — each context workspace (all of its capacity, on every call that
                                     carves it, grown or not), the public-input table in front of its upload, the proof-pack map
                                     where it is rebuilt, and (process default only) the per-call device temporaries of the
                                     host-pointer probes and convenience forms (rsv_poseidon2_permute, rsv_verify_batch,
                                     rsv_verify_hints, ...) as each is allocated.  Left alone: tables that are uploaded whole
                                     (twiddles, programs, wires), the caller's own scratch, and the device slots that
                                     rsv_verify_batch_host and the multi-GPU contexts keep between calls (blob, offsets, verdicts,
                                     bitmap: they hold a call's own uploads and outputs, no intermediate state).  A
                                     result that changes under any fill byte read a word
                                     the call did not write.  It SYNCHRONISES: each fill waits on the host for all three streams of
                                     the context and for the fill itself, so no entry point's "no host synchronisation" holds
                                     while it is set.  Anything else: RSV_E_RANGE */
    /* 15, 27, 28, 29: retired; rsv_ctx_set_option answers RSV_E_SIZE */
    RSV_OPT_CAP_TOP = 19          /* 0 auto (batches of >= 1 024 proofs), 1 the last two or three levels of every Merkle tree in a
                                     kernel of their own (one lane per tree), 2 inside the tree kernels (dense top-of-tree cap) */
} rsv_option;
int rsv_ctx_set_option(rsv_ctx* ctx, int option, long long value);

/* ---- a3: Poseidon2-M31 width-16 permutation -------------------------------
 * Replaces poseidon2_permute (primitives/poseidon31/src/implementation.rs:108-149).
 * n states of 16 words, state-major (state i at in16 + 16*i). */
int rsv_poseidon2_permute(const uint32_t* in16, uint32_t* out16, size_t n, int device);
/* Device-resident form: enqueued on the context's stream, no host round trip.  Inputs >= P are still permuted
 * (as canonical-mod-P garbage); if d_bad (device u32, may be NULL) is given it is set to 1 when any input word
 * was not canonical and left untouched otherwise — the caller zeroes it and reads it when it synchronises. */
int rsv_poseidon2_permute_dev(rsv_ctx* ctx, const uint32_t* d_in16, uint32_t* d_out16, size_t n, uint32_t* d_bad);

/* ---- a4: Poseidon2HalfVar::permute with swap / rate / capacity ------------
 * Replaces Poseidon2HalfVar::permute(left,right,_,_,is_swap)
 * (primitives/poseidon31/src/lib.rs:282-423), values only.
 * For each i: state = swap[i] ? right_i||left_i : left_i||right_i; permute;
 * out_rate8 = state[0..8], out_cap8 = state[8..16].  swap, out_rate8 or
 * out_cap8 may be NULL (no swap / result ignored). */
int rsv_poseidon2_half_permute(const uint32_t* left8, const uint32_t* right8,
                               const uint8_t* swap, uint32_t* out_rate8,
                               uint32_t* out_cap8, size_t n, int device);

/* ---- f4: gate values of the emulated Poseidon2 ------------------------------
 * Replaces the value side of poseidon_permute_emulated(left, right, is_swap)
 * (primitives/poseidon31/src/emulated.rs:80-221): the permutation written as M4 / pow5m4 / pow5 / Hadamard /
 * grand-sum / add / mul gates of the Plonk-without-Poseidon constraint system
 * (constraint_system/src/plonk_without_poseidon.rs:113-305).  For each of n permutations, rows receives the QM31
 * value of every variable the gadget appends to the circuit's witness, in allocation order, for a circuit whose
 * constants are already cached (primitives/fields/src/qm31.rs:39-73: every call but a circuit's first):
 *   rows[p][0 .. 12)    the swap gates, present when is_swap = Some(..) and zero when it is None
 *   rows[p][12 .. 413)  the 401 variables of the permutation itself; rows[p][409 .. 413) are the output state
 *                       (left half in the first two)
 *   rows[p][413 .. 416) zero: padding to RSV_EMU_STRIDE rows, so that each permutation's rows are 52 whole 128-byte
 *                       lines (the kernel is bound by HBM writes and stores whole aligned lines)
 * left8 / right8: n x 8 canonical words (a half = two QM31 of four words each).  swap: NULL (all None) or n bytes,
 * 0 = None, 1 = Some((false, _)), 2 = Some((true, _)); other values or words >= P give RSV_E_RANGE. */
#define RSV_EMU_SWAP_ROWS 12
#define RSV_EMU_ROWS 413
#define RSV_EMU_STRIDE 416
int rsv_poseidon2_emulated(const uint32_t* left8, const uint32_t* right8, const uint8_t* swap,
                           uint32_t* rows /* [n][RSV_EMU_STRIDE][4] */, size_t n, int device);
/* Device-resident form on the context's stream.  d_left8 / d_right8 / d_rows must be 16-byte aligned (d_rows on a
 * 128-byte line for full speed).  d_bad
 * (device u32, may be NULL) is set to 1 on a range error and left untouched otherwise, as for
 * rsv_poseidon2_permute_dev. */
int rsv_poseidon2_emulated_dev(rsv_ctx* ctx, const uint32_t* d_left8, const uint32_t* d_right8, const uint8_t* d_swap,
                               uint32_t* d_rows, size_t n, uint32_t* d_bad);

/* ---- a5: Poseidon31 Merkle hasher -----------------------------------------
 * Replaces Poseidon31MerkleHasherVar::{hash_tree, hash_tree_with_column,
 * hash_m31_columns_get_rate, ...} (primitives/merkle/src/lib.rs:9-181) ==
 * stwo Poseidon31MerkleHasher::hash_node(children, columns).
 * n nodes; node i has children left8+8*i / right8+8*i (both NULL => leaves)
 * and n_cols column words at cols + n_cols*i (n_cols may be 0 iff children given). */
int rsv_merkle_hash_node(const uint32_t* left8, const uint32_t* right8,
                         const uint32_t* cols, size_t n_cols, uint32_t* out8,
                         size_t n, int device);

/* ---- a1 / a2 / a8 / last layer of a12: arithmetic probes ------------------------
 * The device functions the verify kernels are built from, exposed one lane per item so that a binding (and the
 * parity tests) can check them in isolation.  Elements are QM31 = 4 words (a0, a1, b0, b1) = (a0 + a1 i) +
 * (b0 + b1 i) u, all canonical (else RSV_E_RANGE).
 *   RSV_F_QADD/QSUB/QMUL  out = a (+,-,*) b                    primitives/fields/src/qm31.rs:87-249
 *   RSV_F_QINV            out = 1/a                            qm31.rs:360-366
 *   RSV_F_MMUL / MINV     first word only: a0*b0, 1/a0         primitives/fields/src/m31.rs:62-115,140-156
 *   RSV_F_CMUL / CINV     first two words: CM31 product, 1/a   primitives/fields/src/cm31.rs:87-192
 *   RSV_F_QMULI / QMULU   a*i, a*u                             qm31.rs:402-418
 *   RSV_F_QPOW            a ^ (first word of b, any u32)       qm31.rs (QM31Var::pow; test :489)
 * b4 may be NULL for the unary operations. */
enum { RSV_F_QADD = 0, RSV_F_QSUB, RSV_F_QMUL, RSV_F_QINV, RSV_F_MMUL, RSV_F_MINV, RSV_F_CMUL, RSV_F_CINV,
       RSV_F_QMULI, RSV_F_QMULU, RSV_F_QPOW };
int rsv_field_op(int op, const uint32_t* a4, const uint32_t* b4, uint32_t* out4, size_t n, int device);
/* a8: xy[2i], xy[2i+1] = CanonicCoset(log_size).circle_domain().at(bit_reverse(q[i], log_size)) — the point
 * PointCarryingQueryVar carries for position q[i] (primitives/query/src/lib.rs:57-168, circle/src/lib.rs:44-131;
 * reference test circle/src/lib.rs:264).  q[i] is masked to log_size bits; 1 <= log_size <= 30. */
int rsv_domain_points(uint32_t log_size, const uint32_t* q, uint32_t* xy, size_t n, int device);
/* a10 on its own: the OODS composition evaluation of CompositionCheck::compute
 * (components/recursive/composition/src/lib.rs:60-120, plonk.rs:8-82, poseidon.rs:73-241) for n items.
 *   samples4  [n][142][4]  the sampled values, flattened tree-major / column-major / sample-minor
 *   params26  [n][26]      log_size_plonk, log_size_poseidon (1..28), plonk_total_sum, poseidon_total_sum, z, alpha,
 *                          random_coeff, oods_point.x                          (QM31 = 4 words each)
 *   out8      [n][8]       the accumulator over the 86 constraints | left + right * pi^(bound-2)(x): the proof passes
 *                          the composition check iff the two are equal */
int rsv_oods_eval(const uint32_t* samples4, const uint32_t* params26, uint32_t* out8, size_t n, int device);
/* The last-layer comparison of FoldingResults::compute (components/recursive/folding/src/lib.rs:194-204) on its own:
 * ok[i] = 1 iff the polynomial (2^log_n QM31 coefficients) evaluated at x[i] equals folded4[i] — the device function
 * whose failure is RSV_R_FRI_LAST, a reason no mutated proof reaches (the polynomial is hashed before the proof of
 * work, so every mutation stops earlier). */
int rsv_last_layer_check(const uint32_t* coeffs4, uint32_t log_n, const uint32_t* x, const uint32_t* folded4, uint8_t* ok,
                         size_t n, int device);
/* LinePolyVar::eval_at_point (primitives/line/src/lib.rs:39-67; reference test :82): one polynomial of 2^log_n
 * QM31 coefficients (log_n <= 16) evaluated at n points x[i] (M31). */
int rsv_line_eval(const uint32_t* coeffs4, uint32_t log_n, const uint32_t* x, uint32_t* out4, size_t n, int device);

/* ---- a9: one authentication path per query --------------------------------
 * Replaces SinglePathMerkleProofVar::verify
 * (components/recursive/data_structures/src/lib.rs:315-354).
 * n independent paths of equal `depth`; path i: query position query[i],
 * siblings sib8 + 8*depth*i (leaf level first), column words laid out per
 * level: level h (depth..0) has n_cols_at[h] words for every path, packed
 * level-major from the leaf level down (cols + i*sum(n_cols_at)).
 * out_root8 receives the recomputed root (8 words per path). */
int rsv_merkle_path_root(const uint32_t* query, const uint32_t* sib8,
                         const uint32_t* cols, const uint32_t* n_cols_at /* depth+1 */,
                         uint32_t depth, uint32_t* out_root8, size_t n, int device);

/* ---- a6/a7: Fiat-Shamir transcript (parity probe) -------------------------
 * Replaces FiatShamirResults::compute (components/recursive/fiat_shamir/src/lib.rs:31-176).
 * out layout (u32 words):
 *   [0]      reason after transcript stage (RSV_R_OK / PARSE / POW)
 *   [1]      n_fri_alphas = 1 + n_inner_layers
 *   [2]      n_queries
 *   [3]      M = log size of the largest committed column (query bits)
 *   [4..8)   z          [8..12)  alpha       [12..16) random_coeff
 *   [16..20) oods_t     [20..24) oods.x      [24..28) oods.y
 *   [28..32) after_sampled_values_random_coeff
 *   [32..40) channel digest after the proof-of-work mix
 *   [40..40+4*n_fri_alphas)  fri alphas
 *   then n_queries raw query words (before masking to M bits).
 * Returns RSV_E_CAP if cap (in words) is too small.
 * PROBE, not a verdict: it replays the transcript under the configuration words serialized in the proof (no
 * rsv_cfg_set), so word [0] == RSV_R_OK says nothing about the proof's security level. */
int rsv_transcript(const uint8_t* proof, size_t len, uint32_t* out, size_t cap, int device);

/* ---- full verify: a1-a13 --------------------------------------------------
 * Replaces the stage sequence FiatShamirResults::compute →
 * CompositionCheck::compute → AnswerResults::compute → FoldingResults::compute
 * (examples/single-proof/src/main.rs:48-82) on a batch of serialized
 * PlonkWithPoseidonProof<Poseidon31MerkleHasher> (bincode).
 *   blob     concatenated proof bytes; proof i = blob[offsets[i] .. offsets[i+1])
 *   cfg      REQUIRED (RSV_E_NULL otherwise): the configuration(s) the caller expects, see rsv_cfg_set; a proof
 *            whose embedded configuration differs is rejected with RSV_R_PARSE
 *   pi,n_pi  public inputs shared by the whole batch
 *   accept   n bytes, 1 = verified        reason  n bytes of rsv_reason (may be NULL)
 */
int rsv_verify_batch(const uint8_t* blob, const uint64_t* offsets, size_t n,
                     const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi,
                     uint8_t* accept, uint8_t* reason, int device);

/* Same, inputs and outputs resident in HBM (d_ = device pointers); enqueued on ctx's streams.  d_offsets must be 8-byte
 * aligned, d_blob 4-byte aligned and every offset a multiple of 4 (bincode proofs of this type always have
 * 4-byte-multiple lengths).  d_blob needs no padding: no kernel reads a byte at or past d_blob + offsets[n] (every read
 * is bounded by the parser's section lengths, which lie inside the proof's own bytes).
 * Host synchronisation: a batch under ONE configuration (cfg->n_cfgs == 1, cfg_of NULL) is enqueued completely and the
 * call returns without waiting for the device (after the first call has grown the workspaces).  A batch under several
 * configurations is bucketed by n_queries on the host: the call waits for the parser (a few hundred microseconds),
 * reads 8 bytes per proof back, and enqueues the rest; so do the calls with per-query path outputs
 * (rsv_trace_paths_dev, rsv_fri_paths_dev, the path / query-value outputs of rsv_verify_hints_dev), whose declared
 * shape is checked on the host.  Either way the verdicts are complete only after rsv_ctx_synchronize /
 * rsv_stream_wait_ctx. */
int rsv_verify_batch_dev(rsv_ctx* ctx, const uint8_t* d_blob, const uint64_t* d_offsets,
                         size_t n, const rsv_cfg_set* cfg, const rsv_public_input* pi,
                         size_t n_pi, uint8_t* d_accept, uint8_t* d_reason);

/* ---- a batch in which every proof has its own public inputs ---------------------------------------------------------
 * rsv_verify_batch_inputs_dev is rsv_verify_batch_dev with d_pi [n][n_pi] records IN HBM (4-byte aligned), proof i's own
 * inputs at d_pi[i * n_pi .. (i + 1) * n_pi); n_pi is the same for every proof.  Host synchronisation, mixed
 * configurations (cfg_of) and the verdicts are exactly rsv_verify_batch_dev's; a batch under one configuration is
 * enqueued without waiting for the device.  The inputs enter in one place, the logup balance
 *     plonk_sum + poseidon_sum + sum_i 1 / (value_i + (idx_i mod P) alpha - z) = 0        (else RSV_R_LOGUP),
 * whose last term a kernel of its own (one wave per proof, batched inversions) computes per proof behind the transcript
 * and ahead of the OODS check.  Two rules:
 *   - a zero denominator adds nothing, which is what the shared form's per-term inverse (1 / 0 = 0) adds;
 *   - the inputs are in HBM and cannot be refused without a synchronisation: a value word >= P is data.  It counts as 0
 *     and the proof gets RSV_R_PARSE (a non-canonical field element); its neighbours are unaffected.  (The shared form,
 *     and rsv_verify_batch_inputs below, refuse such a word on the host with RSV_E_RANGE.)
 * Given every proof the same records, the call returns rsv_verify_batch_dev's accept and reason byte for byte.
 * Refusals before any device work: a NULL pointer (d_pi may be NULL with n_pi = 0; d_reason may be NULL): RSV_E_NULL;
 * n_pi > 4096, n * n_pi > RSV_MAX_INPUT_RECORDS, a pointer not aligned as above: RSV_E_SIZE.
 * rsv_verify_hints_inputs_dev is the same for rsv_verify_hints_dev; rsv_verify_batch_inputs is the host-memory form of
 * rsv_verify_batch (pi [n][n_pi] host records; a value word >= P: RSV_E_RANGE).
 * Recursing over such a batch: rsv_witness_program_build_inputs, rsv_witness_eval_inputs_dev and
 * rsv_witness_eval_groups_inputs_dev, below.  Not built: per-proof inputs in rsv_verify_batch_host, rsv_multi_* and
 * rsv_exchange_*; a differing n_pi within a batch. */
#define RSV_MAX_INPUT_RECORDS 1073741824 /* 2^30: n * n_pi of the per-proof entry points (the records' words are indexed in 64 bits) */
int rsv_verify_batch_inputs_dev(rsv_ctx* ctx, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, const rsv_cfg_set* cfg,
                                const rsv_public_input* d_pi, size_t n_pi, uint8_t* d_accept, uint8_t* d_reason);
int rsv_verify_batch_inputs(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                            const rsv_public_input* pi, size_t n_pi, uint8_t* accept, uint8_t* reason, int device);
/* The statement sum alone (a per-operation entry point, as rsv_oods_eval): d_sum[i] = sum_k 1 / (value_ik + (idx_ik mod P)
 * alpha_i - z_i) over proof i's n_pi records, (z_i, alpha_i) = d_z_alpha[i][0..3], [4..7].  d_bad [n] (may be NULL): 1 where
 * a value word, or a word of z or alpha, is >= P (the word counts as 0), else 0.  All pointers 4-byte aligned.  Refusals as
 * above, with n <= 2^26.  Enqueued on the context's stream. */
int rsv_public_input_sum_dev(rsv_ctx* ctx, const rsv_public_input* d_pi, size_t n, size_t n_pi, const uint32_t* d_z_alpha,
                             uint32_t* d_sum, uint8_t* d_bad);
/* The digest of the statements a recursion step verifies: eight words whatever the number of proofs and records, for a
 * tree of recursion whose statement must not grow with its depth.  A group is `copies` proofs (a plain batch: copies = 1)
 * with n_own records each, d_pi [n_groups * copies][n_own] in HBM as above; v[c * n_own + k] = value[0] of record k of the
 * group's proof c, T = copies * n_own words, and
 *     digest = Poseidon31MerkleHasherVar::hash_m31_columns_get_rate(v[0 .. T))        (primitives/merkle/src/lib.rs:50-91)
 * which is what rsv_merkle_hash_node(NULL, NULL, v, T, ...) returns: ceil(T / 8) + 1 permutations.  The records' idx is not
 * hashed.  d_stmt [n_groups][8] records: idx = 4 + k, value = (digest[k], 0, 0, 0) — the form the entry points above take,
 * so whoever holds the leaf statements folds them level by level: d_stmt of one level is d_pi (n_own = 8) of the next.
 * d_bad [n_groups] (may be NULL): 1 where a value[0] is >= P (it counts as 0) or a value[1..3] is not 0 (the circuit
 * holds a statement in M31 variables), else 0; the neighbouring groups are unaffected.  Pointers 4-byte aligned.  Small
 * batches run 16 threads per group, large ones a lane per group (RSV_OPT_STATEMENT_ROW_MAX); the result is the same.
 * Refusals before any device work: a NULL pointer (but d_bad): RSV_E_NULL; copies 0 or > 64, n_own 0 or > 4096,
 * n_groups > 2^26, n_groups * copies * n_own > RSV_MAX_INPUT_RECORDS, a pointer not aligned: RSV_E_SIZE.  Enqueued on the
 * context's stream.  The witness program whose statement is this digest: rsv_witness_program_build_inputs_hashed. */
int rsv_statement_digest_dev(rsv_ctx* ctx, const rsv_public_input* d_pi, size_t n_groups, size_t copies, size_t n_own,
                             rsv_public_input* d_stmt, uint8_t* d_bad);

/* Proofs that start in HOST memory, as the reference's callers hold them: one serialized buffer per proof
 * (bincode::serialize(&proof) -> Vec<u8>, examples/multi-proofs/src/main.rs:69-139).  Chunks of about
 * RSV_OPT_HOST_CHUNK_MB (default 256) MB are gathered into pinned staging memory by worker threads
 * (RSV_OPT_HOST_THREADS, default min(cores, 4)), uploaded by the DMA engine and verified, the three stages overlapping
 * (a job below eight such chunks is cut into eight, none under 32 MB, so that the pipeline has something to overlap);
 * accept / reason are host arrays of n bytes.  Blocks until every verdict is written.  A buffer whose length is not a
 * multiple of 4 (every proof of this type is a whole number of 32-bit words) or exceeds 32 MB (a well-formed proof is
 * below 8 MB) is not uploaded and gets RSV_R_PARSE, like any other malformed proof. */
int rsv_verify_batch_host(rsv_ctx* ctx, const uint8_t* const* proofs, const uint64_t* lens, size_t n,
                          const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint8_t* accept,
                          uint8_t* reason);
/* Pinned host memory for proofs.  A caller that can cooperate reads / deserialises its proofs straight into such an
 * arena, back to back in job order: rsv_verify_batch_host (and rsv_multi_verify_batch_host) then recognise every chunk
 * whose proofs lie contiguously inside one arena and let the DMA engine upload it from where it is — no gather copy, no
 * staging ring (the pinned ring is not even allocated when the whole job qualifies).  Anything else (pageable memory,
 * gaps, proofs out of order) goes through the gather as before; the two mix freely chunk by chunk.  hipHostMalloc is
 * slow (about 1 GB/s): allocate once, reuse.  rsv_host_free ignores pointers this library did not hand out. */
int rsv_host_alloc(size_t bytes, void** out);
void rsv_host_free(void* p);

/* ---- SURVEY 8f.1 (next row): per-query authentication paths -----------------
 * Emits, while verifying, the per-query Merkle paths of the four commitment trees in TRANSCRIPT query order —
 * the data SinglePathMerkleProof::from_stwo_proof (components/hints/src/decommit.rs:44-183) derives on the host
 * by re-hashing stwo's batched decommitment.  All n proofs must share one shape: n_queries (>= 4) and
 * max_log = M (log size of the largest column) as declared by the caller, else RSV_E_SIZE.
 *   d_sib  [n][4][n_queries][max_log][8]  sibling hash at the k-th level above the leaf of tree t at index k
 *                                         (entries beyond the tree's depth are not written)
 *   d_pos  [n][4][n_queries]              position of the query at the tree's leaf level
 * Tree depths: max(lp, lq) + log_blowup for trees 0..2, M for tree 3.  accept/reason as in rsv_verify_batch_dev. */
int rsv_trace_paths_dev(rsv_ctx* ctx, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                        const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint32_t n_queries, uint32_t max_log,
                        uint32_t* d_sib, uint32_t* d_pos, uint8_t* d_accept, uint8_t* d_reason);
/* Same on host buffers (copied to `device` and back). */
int rsv_trace_paths(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                    const rsv_public_input* pi, size_t n_pi,
                    uint32_t n_queries, uint32_t max_log, uint32_t* sib, uint32_t* pos, uint8_t* accept,
                    uint8_t* reason, int device);

/* Same for the FRI trees: the per-query pair paths SinglePairMerkleProof::from_stwo_proof
 * (components/hints/src/folding.rs:93-287) derives on the host.  Tree s = 0 is the first layer (leaf level
 * M = max_log, one QM31 column at each distinct column log size), s = 1 + i inner layer i (leaf level M - 1 - i).
 * The batch must share (n_queries >= 4, max_log, n_inner), else RSV_E_SIZE.
 *   d_sib  [n][1 + n_inner][n_queries][max_log][8]  sibling_hashes[k], k = 0..depth-2: at level depth-1-k the
 *                                                   sibling's hash, or — where that level carries a column —
 *                                                   the hash of the sibling's children
 *   d_cols [n][1 + n_inner][n_queries][3][8]        c-th column level from the top: self value | sibling value */
int rsv_fri_paths_dev(rsv_ctx* ctx, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                      const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint32_t n_queries, uint32_t max_log, uint32_t n_inner,
                      uint32_t* d_sib, uint32_t* d_cols, uint8_t* d_accept, uint8_t* d_reason);
int rsv_fri_paths(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                  const rsv_public_input* pi, size_t n_pi,
                  uint32_t n_queries, uint32_t max_log, uint32_t n_inner, uint32_t* sib, uint32_t* cols, uint8_t* accept,
                  uint8_t* reason, int device);

/* ---- everything the reference's hint structs need, from ONE verifying pass ------------------------
 * rsv_verify_hints_dev = rsv_verify_batch_dev that also writes whichever of these outputs are non-NULL:
 *   d_transcript [n][RSV_TRANSCRIPT_WORDS]  per proof, what FiatShamirHints (components/hints/src/fiat_shamir.rs:69-256)
 *                                           carries: words [0..40) as rsv_transcript's; [40..40+4*29) the FRI alphas
 *                                           (first layer, then inner layers; zero padded); [156..284) the raw query
 *                                           words in transcript order (zero padded).  Mixed shapes allowed.
 *   d_trace_sib / d_trace_pos               as rsv_trace_paths_dev   (both or neither)
 *   d_trace_cols [n][4][n_queries][64]      optional (with or without d_trace_sib): SinglePathMerkleProof::columns — the query's
 *                                           column values at the leaf level, then those at the lower column log size
 *                                           (the packing rsv_merkle_path_root takes)
 *   d_fri_sib / d_fri_cols                  as rsv_fri_paths_dev     (both, or d_fri_cols alone)
 *   d_fri_folded [n][3][n_queries][4]       optional, with d_fri_sib: FirstLayerHints::folded_evals_by_column
 *                                           (components/hints/src/folding.rs:291-293) — the circle-to-line fold of
 *                                           each query's first-layer pair at the c-th column log size (descending)
 *   d_query_values [n][n_queries][4*(8+n_inner)]  optional parity probe of rows a11 / a12 (values, not only verdicts),
 *                                           per query in transcript order, QM31 each: the DEEP-quotient answers at
 *                                           the (up to 3) column log sizes, descending (answer/src/lib.rs:294-315);
 *                                           their circle-to-line folds (folding/src/lib.rs:57-90); the value entering
 *                                           inner layer i, i < n_inner (:135-144); the value entering the last-layer
 *                                           check and the last-layer polynomial evaluated at the query's point (:194-204)
 *                                           (the library zeroes this buffer first: absent groups, and the rows of a proof
 *                                           the parser rejected, are zero; a proof rejected behind the parser keeps what
 *                                           its failing verification computed, as its flow records do)
 * Path outputs need a uniform batch of the declared shape (n_queries >= 4, max_log, n_inner), else RSV_E_SIZE.
 *
 * SURVEY 8f.1, second half — the value side of the recursion circuit's Poseidon accelerator:
 *   d_flow       [n][flow_stride][32]  PoseidonFlow (constraint_system/src/plonk_with_poseidon.rs:36,117-128,468-519) of
 *                                      the circuit that verifies proof i: one record per Poseidon2HalfVar::permute
 *                                      invocation (primitives/poseidon31/src/lib.rs:282-423) = the hash words of the four
 *                                      PoseidonEntry: left8 | right8 (the inputs as given; the accelerator applies
 *                                      the swap) | out_rate8 | out_cap8 — one 128-byte line per record; 16-byte aligned
 *   d_flow_swap  [n][flow_stride]      SwapOption::swap of the record (bytes; both or neither with d_flow)
 *   d_flow_count [n]                   optional: records of proof i = rsv_poseidon_flow_count of its shape; 0 when the
 *                                      parser rejected it or flow_stride is too small for it (nothing is written then)
 *   flow_stride                        records the caller allocated per proof
 * Record order = the circuit's invocation order (examples/multi-proofs/src/main.rs:69-139): every channel operation of
 * FiatShamirResults::compute (including the ceil(n_queries / 4) query draws the circuit makes where ceil(n_queries / 8)
 * hold every query); then, for each of the four commitment trees, one SinglePathMerkleProofVar::verify per query in
 * TRANSCRIPT query order (components/recursive/answer/src/lib.rs:214-258, data_structures/src/lib.rs:315-354); then one
 * SinglePairMerkleProofVar::verify per query for the first FRI layer and for every inner layer
 * (folding/src/lib.rs:23-33,186-189, data_structures/src/lib.rs:400-464).  What a next-level prover pads to a multiple of
 * 16 and proves as its Poseidon component (six trace rows per record).  Any mix of shapes; the records of a proof
 * that is rejected behind the parser are whatever its (failing) verification computed.  With d_flow the per-query
 * kernels walk every path to the root themselves (no shared top-of-tree cap, no shared row hashes), like the circuit.
 * PINNED value by value through the fixture chain: the circuit that verifies fixture K, rebuilt from these records and the
 * witness below, evaluated at fixture K+1's OODS point, gives K+1's sampled values (tests/test_witness_gpu.py: the GPU's
 * own flow reproduces the next fixture's 88 Poseidon columns for all 14 pairs; oracle/recursion_circuit).  The wire
 * indices of PoseidonEntry / SwapOption::addr are constants of the shape: rsv_witness_program_export (flow_wires). */
#define RSV_TRANSCRIPT_WORDS 284
typedef struct {
    uint32_t n_queries, max_log, n_inner; /* declared common shape; ignored when no path output is requested */
    uint32_t* d_transcript;
    uint32_t* d_trace_sib;
    uint32_t* d_trace_pos;
    uint32_t* d_trace_cols;
    uint32_t* d_fri_sib;
    uint32_t* d_fri_cols;
    uint32_t* d_fri_folded;
    uint32_t* d_query_values;
    /* PoseidonFlow (ABI v3), see above */
    uint32_t* d_flow;
    uint8_t* d_flow_swap;
    uint32_t* d_flow_count;
    uint32_t flow_stride;
    /* the batch's accept bitmap and count from the verifying pass (ABI v3): what rsv_accept_bitmap_dev computes from
     * the accept bytes, written by the kernel that writes the verdicts (one launch less on the latency path of a
     * small batch).  d_accept_bitmap: ceil(n/32) words; d_accept_count: optional u64, needs d_accept_bitmap. */
    uint32_t* d_accept_bitmap;
    uint64_t* d_accept_count;
} rsv_hints_out;
int rsv_verify_hints_dev(rsv_ctx* ctx, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                         const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, const rsv_hints_out* out, uint8_t* d_accept,
                         uint8_t* d_reason);
/* rsv_verify_hints_dev on a batch in which every proof has its own public inputs: d_pi [n][n_pi] in HBM, as
 * rsv_verify_batch_inputs_dev takes them, with its rules and refusals. */
int rsv_verify_hints_inputs_dev(rsv_ctx* ctx, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, const rsv_cfg_set* cfg,
                                const rsv_public_input* d_pi, size_t n_pi, const rsv_hints_out* out, uint8_t* d_accept,
                                uint8_t* d_reason);
/* Same with every pointer (blob, offsets, the outputs named in *out, accept, reason) in HOST memory: the library
 * stages them through HBM.  rsv_trace_paths, rsv_fri_paths and rsv_transcript_batch are special cases of it. */
int rsv_verify_hints(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                     const rsv_public_input* pi, size_t n_pi,
                     const rsv_hints_out* out, uint8_t* accept, uint8_t* reason, int device);
/* Records in the PoseidonFlow of one proof with these component log sizes under cfg (pure arithmetic, no device). */
int rsv_poseidon_flow_count(uint32_t log_size_plonk, uint32_t log_size_poseidon, const rsv_pcs_config* cfg, uint32_t* count);
/* Host-buffer convenience for the transcript rows only (any mix of shapes): out is [n][RSV_TRANSCRIPT_WORDS]. */
int rsv_transcript_batch(const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg, uint32_t* out,
                         int device);

/* ---- SURVEY 8f.1, completed: the recursion circuit's witness ------------------------------------------------------
 * What the reference's circuit leaves for the next prover is `variables: Vec<QM31>`
 * (constraint_system/src/plonk_with_poseidon.rs:19): one value per cs.add / cs.mul / cs.mul_constant / new_m31 /
 * new_qm31 call of the gadgets, in call order (:140-283); the trace columns a_val / b_val / c_val are that vector read
 * through the wires (:571-618).  The reference computes it by running the gadgets on one proof at a time on the CPU.
 * Which gate or hint produces variable k is the same for every proof of one shape (statement sizes + PcsConfig), so
 * here the gadgets are run once per shape on the host (rsv_witness_program_build: csrc/circuit_*.hpp, a mirror of the
 * reference's ConstraintSystemRef / M31Var / ... / FiatShamirResults / CompositionCheck / AnswerResults / FoldingResults
 * that writes down what it did) and the resulting PROGRAM — one instruction per variable, sorted by dependency depth — is evaluated
 * on the GPU for a whole batch, from the hints of the verifying pass (proof words, PoseidonFlow records, per-query
 * column values).  The circuit is `copies` copies of the verifier in one constraint system, as
 * examples/multi-proofs/src/main.rs:66-139 builds it (`multipliers`).  Under rsv_witness_eval_dev every copy verifies the
 * same proof, as in that example; under rsv_witness_eval_groups_dev copy c verifies the c-th proof of a group of `copies`
 * proofs of one shape (aggregation).
 *
 * Instruction = 8 u32: op, dst, a, b, imm0..imm3 (ops: recursive-stwo_amd/csrc/k_witness.hpp WitnessOp; the table with
 * their meaning heads recursive-stwo_amd/witness_program.py).  rsv_witness_program_create checks every index the device
 * will use (RSV_E_RANGE otherwise) and keeps a copy in HBM. */
typedef struct rsv_witness_program rsv_witness_program;
typedef struct {
    uint32_t log_size_plonk, log_size_poseidon;            /* the statement of the proofs the program applies to */
    uint32_t pow_bits, log_blowup, log_last, n_queries;    /* their PcsConfig */
    uint32_t n_inner;                                      /* FRI inner layers */
    uint32_t flow_count;                                   /* rsv_poseidon_flow_count of the shape */
    uint32_t copies;                                       /* copies of the verifier in the circuit */
} rsv_witness_shape;
int rsv_witness_program_create(const uint32_t* instr, size_t n_instr, const uint32_t* level_offsets, size_t n_levels,
                               uint32_t n_vars, const rsv_witness_shape* shape, int device, rsv_witness_program** out);
void rsv_witness_program_destroy(rsv_witness_program* prog);
/* The program of the shape of `proof` (a template: any proof of that shape that verifies under cfg with these public
 * inputs, else RSV_E_RANGE), for a circuit of `copies` copies of the verifier: runs the library's mirror of the
 * reference's gadgets (csrc/circuit_{cs,gadgets,verifier}.hpp: ConstraintSystemRef, M31Var .. QM31Var, BitsVar,
 * Poseidon2HalfVar, ChannelVar, the Merkle hasher, circle points, LinePolyVar, query positions; PlonkWithPoseidonProofVar,
 * FiatShamirResults, CompositionCheck, AnswerResults, FoldingResults) once over the template on the host, fed with the
 * hints of the GPU's verifying pass over it.  A few milliseconds per 50 000 variables, plus that one verifying pass.
 * set_walks (NULL = all zero): one byte per copy.  AnswerResults::compute walks two std HashSet<isize> = {0, -1} whose
 * order Rust seeds per process (components/recursive/answer/src/lib.rs:44-71), so the reference's own circuit comes in
 * four variants per copy that differ in the ORDER of two pairs of blocks of variables (the values are the same); bit 0 =
 * the Plonk set is walked -1 first, bit 1 = the Poseidon set.  A prover that already fixed its gate list (preprocessed
 * columns) passes the walks that list was made with.  A PROVER INTEGRATION MUST DO SO: the library cannot observe which of
 * the four orders a given run of the reference took (the tests recover them per fixture pair by trying the four against the
 * next fixture's sampled values, tests/pin_recursion_circuit.py); with the wrong walks every value is still right but two
 * pairs of blocks of `variables` sit in the other order than the prover's wires expect.
 * The builder also records which copy allocated every variable (one byte each, kept with the program for
 * rsv_witness_eval_groups_dev) and checks that every hint lies in the contiguous range of its own copy: RSV_E_RANGE
 * otherwise (a fault of the library's mirror of the gadgets, never of the template). */
int rsv_witness_program_build(const uint8_t* proof, size_t len, const rsv_pcs_config* cfg, const rsv_public_input* pi, size_t n_pi,
                              uint32_t copies, const uint8_t* set_walks, int device, rsv_witness_program** out);
/* PER-PROOF PUBLIC INPUTS.  rsv_witness_program_build makes every public input a constant of the program, so a program fits
 * one statement.  rsv_witness_program_build_inputs is the same builder with pi[0 .. n_fixed) constants of the program and
 * pi[n_fixed .. n_pi) the proof's OWN inputs (n_own = n_pi - n_fixed <= 4096; n_fixed > n_pi: RSV_E_SIZE): each becomes a
 * PublicInput variable of the circuit (constraint_system/src/plonk_with_poseidon.rs:236-252), so the gate list is the same
 * for every statement, one program serves a batch of proofs that differ in their own inputs (rsv_witness_eval_inputs_dev),
 * and the next proof carries the inner statement as part of its own.  The reference wants public inputs allocated before
 * anything else, so all of them come first: record k of the proof copy c verifies is variable 4 + c * n_own + k, with the
 * row (v, 0, v, op 1, poseidon_wire 0, enforce_c_m31 1) and the instruction W_INPUT, imm0 = k; num_input (rsv_circuit_program_num_input)
 * is 3 + copies * n_own.  A record's idx stays a constant of the program.  `pi` holds the template's own values.
 * THE REFERENCE'S QUIRK STANDS: a PublicInput row enforces M31, so only a statement whose own values are M31 (words 1..3
 * zero) can be recursed; one with a non-zero word 1..3 cannot, and rsv_witness_eval_inputs_dev rejects its proof.
 * With n_fixed == n_pi the program is rsv_witness_program_build's: _info, _export and _gates give the same bytes.
 * rsv_witness_program_inputs: the counts a built program was made for and idx_out [n_own] = the own records' idx (any
 * pointer may be NULL; RSV_E_SIZE for a program made from instructions or from a circuit, which has them not on record).
 * rsv_witness_program_create accepts W_INPUT with imm0 < 4096 (RSV_E_RANGE otherwise). */
int rsv_witness_program_build_inputs(const uint8_t* proof, size_t len, const rsv_pcs_config* cfg, const rsv_public_input* pi, size_t n_pi,
                                     size_t n_fixed, uint32_t copies, const uint8_t* set_walks, int device, rsv_witness_program** out);
int rsv_witness_program_inputs(const rsv_witness_program* prog, uint32_t* n_fixed, uint32_t* n_own, uint32_t* idx_out);
/* A HASHED STATEMENT.  With rsv_witness_program_build_inputs the outer proof carries every inner record: num_input = 3 +
 * copies * n_own, and a tree of recursion multiplies it at every level.  rsv_witness_program_build_inputs_hashed (the same
 * arguments; n_own == 0: RSV_E_SIZE; a template whose own value is no M31: RSV_E_RANGE) builds the circuit whose statement
 * is the DIGEST of the statements it verified (rsv_statement_digest_dev), eight words whatever copies and n_own are.  In
 * allocation order:
 *   variables 4 .. 11: eight PublicInput M31 variables, instruction W_STMT (imm0 = the word), num_input = 11;
 *   the own records: T = copies * n_own M31 WITNESS variables 12 .. 12 + T, copy-major, instruction W_INPUT (imm0 = k) — the
 *     row enforces M31, so a record with a non-zero word 1..3 is still RSV_R_PARSE at evaluation;
 *   half_equalverify(half_from_m31(variables 4 .. 11), hash_m31_columns_get_rate(own records));
 *   the copies of the verifier, as rsv_witness_program_build_inputs runs them, each on its n_own variables.
 * The hash costs S = ceil(T / 8) + 1 Poseidon invocations (swap 0), which the verifying pass cannot produce.  They take
 * the flow indices BEHIND the copies' — flow_wires is [copies * flow_count + S][5], a W_FLOW of the hash has imm0 >= copies *
 * flow_count — and their records lie at the TAIL of the flow buffers: d_flow / d_flow_swap of a hashed program hold the
 * members' records, [n_groups * copies][flow_count] as for any program, followed by [n_groups][S]; circuit flow index i of
 * group g is record g * copies * flow_count + i for i < copies * flow_count, and n_groups * copies * flow_count + g * S + (i -
 * copies * flow_count) otherwise.  The evaluating calls write them (the digest kernel runs ahead of the witness kernels, no
 * host synchronisation) and rsv_witness_trace_dev and its successors read them there; W_STMT k of row g is word k of the
 * group's digest.  The statement of the outer proof is then rsv_circuit_inputs_dev's eleven records, of which 4 .. 11 are
 * what rsv_statement_digest_dev gives for the inner statements.  rsv_witness_eval_inputs_dev takes a hashed program of one
 * copy, rsv_witness_eval_groups_inputs_dev of any number (several copies hash a group's statements: RSV_E_SIZE from the
 * former); the calls without per-proof inputs refuse it as they refuse any program with own inputs.
 * rsv_witness_program_statement: hashed = 1 for such a program (else 0, and the others 0), n_words = 8, stmt_flow_count = S
 * (any pointer may be NULL).  The builder runs the digest kernel once on the template's own records, on a context it makes
 * and destroys for the call (the build needs the device anyway: the template's hints come from a verifying pass).
 * rsv_witness_program_create accepts W_STMT with imm0 < 8 (a program made from instructions has
 * no tail: the op yields zero). */
int rsv_witness_program_build_inputs_hashed(const uint8_t* proof, size_t len, const rsv_pcs_config* cfg, const rsv_public_input* pi,
                                            size_t n_pi, size_t n_fixed, uint32_t copies, const uint8_t* set_walks, int device,
                                            rsv_witness_program** out);
int rsv_witness_program_statement(const rsv_witness_program* prog, uint32_t* hashed, uint32_t* n_words, uint32_t* stmt_flow_count);
/* Sizes, then the arrays (any pointer may be NULL): instr [n_vars][8], level_offsets [n_levels + 1], flow_wires
 * [copies * flow_count][5] = PoseidonEntry::wire of r1..r4 and SwapOption::addr of every invocation (constants of the
 * shape; known to built programs and to those made from a circuit, RSV_E_SIZE otherwise) — what
 * rsv_witness_program_create takes back. */
int rsv_witness_program_info(const rsv_witness_program* prog, uint32_t* n_vars, uint32_t* n_levels, rsv_witness_shape* shape);
int rsv_witness_program_export(const rsv_witness_program* prog, uint32_t* instr, uint32_t* level_offsets, uint32_t* flow_wires);
/* The circuit's gate list as the gadgets left it, or as rsv_circuit_program_create took it (RSV_E_SIZE for a program made
 * from instructions alone): gates [n_rows][6] =
 * a_wire, b_wire, c_wire, op, poseidon_wire, enforce_c_m31 per Plonk row (plonk_with_poseidon.rs:23-36, before pad()) —
 * with `variables` and the flow everything generate_plonk_with_poseidon_circuit (:522-629) and populate_logup_arguments
 * (:345-466) read.  The rows are constants of the shape EXCEPT `op` at the rows listed in witness_ops [n][3] = (row, bit
 * variable, constant): CirclePointM31Var::select takes its gate constant from the selected value
 * (primitives/circle/src/lib.rs:83-98), so there op = constant where the proof's variables[bit] is 1 and 0 where it is 0;
 * `gates` holds the template's.  Call with NULL arrays for the two counts first. */
int rsv_witness_program_gates(const rsv_witness_program* prog, uint32_t* n_rows, uint32_t* n_witness_ops, uint32_t* gates,
                              uint32_t* witness_ops);
/* HBM the context will hold for a batch of n proofs (hints of the verifying pass + variables[var][proof]). */
int rsv_witness_scratch_bytes(const rsv_witness_program* prog, size_t n, size_t* bytes);
/* Verifies the batch (as rsv_verify_hints_dev, under cfg = the program's single configuration, else RSV_E_SIZE) and
 * writes d_variables [n][n_vars][4]: row i = the `variables` vector of the circuit that verifies proof i
 * ([n_vars][n][4] under RSV_OPT_WITNESS_LAYOUT = 2).
 * d_accept[i] = 1 iff proof i verified AND is of the program's shape; only those rows are defined (the others are
 * unspecified).  d_variables 16-byte aligned.
 * d_flow [n][flow_count][32] + d_flow_swap [n][flow_count] (optional, both or neither; as rsv_hints_out::d_flow with
 * flow_stride = the shape's flow_count): the PoseidonFlow of ONE copy of the verifier — the other thing the next prover
 * needs; every copy verifies the same proof here and so invokes the same permutations, the wire indices of invocation k
 * of copy c are the host's (rsv_witness_program_export, flow_wires).  Without them the records live in the context's scratch only. */
int rsv_witness_eval_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                         const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint32_t* d_variables, uint32_t* d_flow,
                         uint8_t* d_flow_swap, uint8_t* d_accept, uint8_t* d_reason);
/* Same on host buffers. */
int rsv_witness_eval(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                     const rsv_public_input* pi, size_t n_pi, uint32_t* variables, uint32_t* flow, uint8_t* flow_swap, uint8_t* accept,
                     uint8_t* reason, int device);
/* AGGREGATION: the batch holds n_groups * copies proofs, group g = proofs [g * copies, (g + 1) * copies) of the blob, and
 * copy c of group g's circuit verifies proof g * copies + c.  As rsv_witness_eval_dev (the same configuration check, the
 * same alignment) with one `variables` vector per GROUP:
 *   d_variables [n_groups][n_vars][4] ([n_vars][n_groups][4] under RSV_OPT_WITNESS_LAYOUT = 2);
 *   d_flow [n_groups][copies][flow_count][32] + d_flow_swap [n_groups][copies][flow_count] (optional, both or neither): the
 *     PoseidonFlow of every member, one proof after the other;
 *   d_accept [n_groups]: 1 iff every member verified and is of the program's shape; only those rows are defined;
 *   d_member_accept, d_member_reason [n_groups * copies]: the members' own verdicts (the reason may be NULL).
 * Built programs only (RSV_E_SIZE otherwise: only the builder knows which copy a hint belongs to); n_groups * copies <= 2^20.
 * With copies == 1 this writes exactly what rsv_witness_eval_dev writes.  rsv_witness_group_scratch_bytes: the HBM the
 * context will hold for n_groups groups (the hints of n_groups * copies proofs + variables[var][group]). */
int rsv_witness_eval_groups_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets,
                                size_t n_groups, const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint32_t* d_variables,
                                uint32_t* d_flow, uint8_t* d_flow_swap, uint8_t* d_accept, uint8_t* d_member_accept,
                                uint8_t* d_member_reason);
int rsv_witness_group_scratch_bytes(const rsv_witness_program* prog, size_t n_groups, size_t* bytes);
/* A batch in which every proof has its own public inputs, for a program with own inputs (rsv_witness_program_build_inputs).
 * rsv_witness_eval_inputs_dev is rsv_witness_eval_dev with pi_fixed [n_fixed]: the shared records (host memory) and d_pi
 * [n][n_own]: proof i's own records IN HBM, 4-byte aligned, as rsv_verify_batch_inputs_dev takes them.  Proof i is
 * verified (rsv_verify_hints_inputs_dev) under the n_fixed shared records followed by its own; the array is assembled on
 * the device, nothing synchronises with the host.  W_INPUT k of row i is d_pi[i][k].value.
 * d_accept[i] = 1 iff proof i verified under its own statement AND is of the program's shape AND every own record's idx is
 * the program's AND every own value is an M31 (words 1..3 zero, word 0 below P).  An idx that differs or a value that is no
 * M31 is RSV_R_PARSE in d_reason[i], as bad statement data is in rsv_verify_batch_inputs_dev.
 * Refused before any device work: a NULL pointer (RSV_E_NULL); n_fixed, n_own or a shared record's idx that differ from
 * what the program was built for, for a program made from instructions a W_INPUT whose imm0 is not below n_own, n * (n_fixed
 * + n_own) > RSV_MAX_INPUT_RECORDS, n_fixed + n_own > 4096, d_pi not 4-byte aligned, a configuration that is not the program's, d_blob or d_offsets not
 * aligned as rsv_verify_batch_dev wants them (RSV_E_SIZE).  With n_own == 0 the
 * call is rsv_witness_eval_dev under pi_fixed.  rsv_witness_eval_dev / rsv_witness_eval_groups_dev refuse a program with
 * own inputs (RSV_E_SIZE).  rsv_witness_eval_inputs: the same on host buffers, pi_own [n][n_own].
 * rsv_witness_eval_groups_inputs_dev is rsv_witness_eval_groups_dev in the same way: d_pi [n_groups * copies][n_own], member
 * g * copies + c brings the records that variables 4 + c * n_own + k of group g hold; a member whose statement the circuit
 * cannot hold is rejected in d_member_accept / d_member_reason, and its group with it. */
int rsv_witness_eval_inputs_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                                const rsv_cfg_set* cfg, const rsv_public_input* pi_fixed, size_t n_fixed, const rsv_public_input* d_pi,
                                size_t n_own, uint32_t* d_variables, uint32_t* d_flow, uint8_t* d_flow_swap, uint8_t* d_accept,
                                uint8_t* d_reason);
int rsv_witness_eval_inputs(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                            const rsv_public_input* pi_fixed, size_t n_fixed, const rsv_public_input* pi_own, size_t n_own,
                            uint32_t* variables, uint32_t* flow, uint8_t* flow_swap, uint8_t* accept, uint8_t* reason, int device);
int rsv_witness_eval_groups_inputs_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint8_t* d_blob, const uint64_t* d_offsets,
                                       size_t n_groups, const rsv_cfg_set* cfg, const rsv_public_input* pi_fixed, size_t n_fixed,
                                       const rsv_public_input* d_pi, size_t n_own, uint32_t* d_variables, uint32_t* d_flow,
                                       uint8_t* d_flow_swap, uint8_t* d_accept, uint8_t* d_member_accept, uint8_t* d_member_reason);

/* ---- a caller's own Plonk-with-Poseidon circuit through the chain -----------------------------------------------------
 * The reference's prove_plonk_with_poseidon proves whatever circuit the constraint system holds; so does the chain from
 * rsv_witness_trace_dev on, which reads of a program only its gate list, flow wires, witness ops and n_vars.
 * rsv_circuit_program_create makes such a program from the circuit itself, in the arrays rsv_witness_program_gates and
 * rsv_witness_program_export return: gates [n_rows][6] (unpadded), flow_wires [n_flow][5], witness_ops [n][3] (may be
 * NULL with a count of 0).  num_input is the reference's: 3 for the constants 1, i, j plus one per new_*(PublicInput); the
 * public inputs are variables 1 .. num_input.  The program has no instructions: shape.copies = 1, shape.flow_count =
 * n_flow, the verifier fields of the shape are zero; _info, _export (instr: nothing is written), _gates and _destroy work
 * on it and every stage of the chain accepts it; what evaluates a witness (rsv_witness_eval*, rsv_witness_scratch_bytes,
 * the host forms rsv_witness_trace / _interaction / _commit, the _groups calls) refuses it with RSV_E_SIZE before any device
 * work.  The witness is the caller's: `variables` [n][n_vars][4], and the flow, which rsv_circuit_flow_dev makes.
 * Host work only (the device copies are uploaded by the first stage that needs them); everything is checked before
 * anything is kept:
 *   RSV_E_NULL   a NULL array with a non-zero count, out NULL;
 *   RSV_E_SIZE   zero rows or flow, a log size beyond RSV_MAX_WITNESS_LOG, n_vars above 2^26;
 *   RSV_E_RANGE  a wire, bit variable or swap address >= n_vars, a witness-op row >= n_rows; the four constant rows
 *                (k, 0, k, op 1) absent; num_input < 3 or >= n_vars; a non-zero flow wire that is not the poseidon_wire of
 *                exactly one row; a Poseidon wire used more than once (the reference's assert in populate_logup_arguments). */
int rsv_circuit_program_create(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow,
                               const uint32_t* witness_ops, size_t n_witness_ops, uint32_t n_vars, uint32_t num_input, int device,
                               rsv_witness_program** out);
/* The reference's two checks before it proves, for n witnesses of one circuit in HBM (d_variables in the layout
 * RSV_OPT_WITNESS_LAYOUT names, 16-byte aligned), for any program with a gate list, built or made from a circuit
 * (RSV_E_SIZE otherwise; RSV_E_RANGE if the program's arrays fail rsv_circuit_program_create's checks).  Enqueued on the
 * context's stream with no host synchronisation; the program's tables go to the device on the first call.
 * d_ok [n] is only ever cleared: the caller sets it to 1, and the same array then serves as the chain's d_accept.  A proof
 * with d_ok[i] == 0 on entry is skipped.  d_bad_row / d_bad_flow [n] are always written: the smallest failing row or
 * invocation, 0xffffffff where there is none or the proof was skipped.
 *   rsv_circuit_check_dev: cs.check_arithmetics() (plonk_with_poseidon.rs:337-381).  Row r fails unless
 *     c == op (a + b) + (1 - op) a b in QM31 (at a witness-op row op = variables[bit].x ? constant : 0), words 1..3 of c are
 *     zero where enforce_c_m31 is set, every word read is below P, and, for r < 4, variable r is 0, 1, i, j.
 *   rsv_circuit_flow_dev: cs.check_poseidon_invocations() (:468-519), and the PoseidonFlow itself.  d_flow
 *     [n][n_flow][32] (16-byte aligned) + d_flow_swap [n][n_flow], in the layout of rsv_hints_out::d_flow, are IN/OUT: an
 *     input half r1 / r2 whose wire is 0 (a previous permutation's ignored output used once) is read from its place in
 *     the record; one with a wire is the pair (variables[a_wire], variables[b_wire]) of the row carrying that
 *     poseidon_wire.  The swap bit is variables[swap address] (address 0: no swap).  The state is r1 || r2, or r2 || r1
 *     under swap; the permutation's output is r3 || r4.  All 32 words and the swap byte of every record are written
 *     (zeros for a skipped proof).  Invocation k fails if a word of its input is not below P, the swap bit is not the
 *     QM31 0 or 1, or an output with a wire differs from its pair in variables. */
int rsv_circuit_check_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_variables, size_t n, uint8_t* d_ok,
                          uint32_t* d_bad_row);
int rsv_circuit_flow_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_variables, size_t n, uint32_t* d_flow,
                         uint8_t* d_flow_swap, uint8_t* d_ok, uint32_t* d_bad_flow);
/* The statement of each of n witnesses in HBM: d_pi [n][num_input] records (k, variables[k]) for k = 1 .. num_input, what
 * rsv_verify_batch_inputs_dev takes for the proofs the chain makes of these witnesses.  d_variables in the layout
 * RSV_OPT_WITNESS_LAYOUT names, 16-byte aligned; d_pi 4-byte aligned.  Any program with a gate list, built (num_input = 3:
 * the constants 1, i, j) or made from a circuit; RSV_E_SIZE otherwise, for a program of another device and for n above
 * 2^20; a NULL pointer: RSV_E_NULL.  Enqueued on the context's stream with no host synchronisation.
 * rsv_circuit_program_num_input: the program's num_input (RSV_E_SIZE for a program without a gate list). */
int rsv_circuit_program_num_input(const rsv_witness_program* prog, uint32_t* num_input);
int rsv_circuit_inputs_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_variables, size_t n, rsv_public_input* d_pi);

/* ---- a caller's circuit evaluated on the GPU: `variables` and the flow from the free inputs ---------------------------
 * rsv_circuit_program_create_eval is rsv_circuit_program_create — the same checks first, with the same statuses, the same
 * program (no verifier instructions: what evaluates the recursion circuit's witness still refuses it) — which beside
 * that compiles the circuit into an EVALUATION program: one definition per variable, and the levels in which
 * rsv_circuit_eval_dev runs them.  The caller then gives, per witness, only n_inputs free QM31 inputs.
 *   hints [n_hints][4] = (dst variable, kind, src variable, imm): what the gate list cannot say.  RSV_HINT_INPUT: dst =
 *     slot `imm` (< n_inputs) of the witness's input buffer; public inputs are ordinary inputs.  The other kinds are the
 *     hints of the reference's gadgets, computed from variable src: COPY dst = src; INV and INV0 dst = (1 / src.x, 0, 0, 0)
 *     with 1 / 0 = 0; QINV dst = 1 / src in QM31 (0 for 0); CINV dst = (coordinate imm (0, 1) of 1 / (src.x + src.y i),
 *     0, 0, 0) (0 for 0); COORD dst = (word imm (0..3) of src, 0, 0, 0); BIT dst = (bit imm (0..31) of src.x, 0, 0, 0).
 *   flow_links [n_flow][2], or NULL for none: the source of an input half r1 / r2 that has no wire.  0: the 8 words the
 *     caller left in d_flow (rsv_circuit_flow_dev's convention); 1 + 2 k' + h': output half h' (0: r3, 1: r4) of invocation
 *     k' — the reference's "ignored output fed to the next permutation", which never becomes a variable.
 * Every variable gets exactly ONE definition, by the first of these rules that applies:
 *   1. variables 0..3 are the constants 0, 1, i, j;
 *   2. a variable that is the dst of a hint is defined by that hint;
 *   3. take the row that carries the poseidon_wire named as r3 or r4 of an invocation: its a_wire is words 0..3 and its
 *      b_wire words 4..7 of that output half (in the reference these are fresh witnesses filled from the permutation);
 *   4. the first row in row order with c_wire == v, a_wire != v and b_wire != v defines v = op (a + b) + (1 - op) a b, where
 *      at a witness-op row op is the row's constant if variables[bit].x != 0 and 0 otherwise.
 * An input half with a wire is (variables[a_wire], variables[b_wire]) of its row, as in rsv_circuit_flow_dev.
 * Instructions and invocations are the nodes of one dependency graph: an instruction depends on the definitions of its
 * operands (at a witness-op row: and of the bit), an invocation on those of its bound input variables, of its swap
 * variable and on its linked invocations, a rule-3 variable on its invocation.  A node's level is the longest path to it;
 * a rule-3 variable is written by its invocation and so is ready with that invocation's level.  No invocation is
 * renumbered: flow record k stays invocation k.
 * Refusals beyond rsv_circuit_program_create's (out is untouched): hints NULL with a count: RSV_E_NULL; n_inputs above
 * 2^26: RSV_E_SIZE; RSV_E_RANGE for a hint's dst or src >= n_vars, an unknown kind, an imm or slot out of range, a hint on
 * a variable 0..3, two hints for one dst, a variable that rule 3 matches twice, a variable without a definition, a link
 * on a half that has a wire, with k' >= n_flow or k' == k, a dependency cycle. */
enum { RSV_HINT_INPUT, RSV_HINT_COPY, RSV_HINT_INV, RSV_HINT_INV0, RSV_HINT_QINV, RSV_HINT_CINV, RSV_HINT_COORD, RSV_HINT_BIT };
int rsv_circuit_program_create_eval(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow,
                                    const uint32_t* witness_ops, size_t n_witness_ops, uint32_t n_vars, uint32_t num_input,
                                    const uint32_t* hints, size_t n_hints, const uint32_t* flow_links, uint32_t n_inputs, int device,
                                    rsv_witness_program** out);
/* The compiled evaluation program (RSV_E_SIZE for a program without one; any pointer may be NULL).  n_instr = n_vars less
 * the rule-3 variables.  _export: instr [n_instr][8] = op, dst, a, b, imm0..3 in rsv_witness_program_create's layout, level
 * after level (ops 0..10 as there; 32: dst = inputs[imm0]; 33: the general gate, op = imm0, or with imm2 = 1 imm0 where
 * variables[imm1].x != 0 and 0 otherwise); level_offsets [n_levels + 1] into instr; flow_order [n_flow], the invocations
 * level after level; flow_level_offsets [n_levels + 1] into flow_order. */
int rsv_circuit_eval_info(const rsv_witness_program* prog, uint32_t* n_inputs, uint32_t* n_levels, uint32_t* n_instr);
int rsv_circuit_eval_export(const rsv_witness_program* prog, uint32_t* instr, uint32_t* level_offsets, uint32_t* flow_order,
                            uint32_t* flow_level_offsets);
/* Evaluates n witnesses of a program made by rsv_circuit_program_create_eval (RSV_E_SIZE otherwise) from d_inputs
 * [n][n_inputs][4] (16-byte aligned): d_variables in the layout RSV_OPT_WITNESS_LAYOUT names, d_flow [n][n_flow][32]
 * (IN/OUT: the input halves with neither a wire nor a link are read from their place) and d_flow_swap [n][n_flow].  For a
 * witness with d_ok[i] != 0 on entry every word of the three is written; a witness skipped on entry is left untouched.
 * An input word >= P clears d_ok[i] and leaves the smallest offending slot in d_bad_input[i] (0xffffffff otherwise; the
 * word counts as 0 in what is written).  The swap bit is variables[swap address].x & 1 (0 for address 0).  The call does
 * not judge satisfiability: rsv_circuit_check_dev and rsv_circuit_flow_dev do, on what this call wrote.  Refusals before
 * any device work: a NULL pointer (d_inputs may be NULL with n_inputs = 0): RSV_E_NULL; a program without an evaluation
 * program or of another device, n above 2^20, a level too wide for one launch at this n, a pointer not 16-byte (d_bad_input:
 * 4-byte) aligned: RSV_E_SIZE.  Enqueued on the context's stream with no host synchronisation; the program's tables go to
 * the device on the first call.  RSV_OPT_CIRCUIT_EVAL_FORM selects between one launch per level and one launch in which a
 * workgroup per witness walks the levels; both write the same words.  The call needs no scratch of the context:
 * rsv_circuit_eval_scratch_bytes answers 0 (RSV_E_SIZE for a program without an evaluation program). */
int rsv_circuit_eval_scratch_bytes(const rsv_witness_program* prog, size_t n, size_t* bytes);
int rsv_circuit_eval_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_inputs, size_t n, uint32_t* d_variables,
                         uint32_t* d_flow, uint8_t* d_flow_swap, uint8_t* d_ok, uint32_t* d_bad_input);

/* ---- the columns the next prover commits: 22 Plonk + 88 Poseidon ----------------------------------------------------
 * generate_plonk_with_poseidon_circuit (constraint_system/src/plonk_with_poseidon.rs:522-629) turns the circuit into the
 * two components of the next proof.  Every column is canonical M31 u32, [column][row], rows in the order the prover holds
 * them (position i = the i-th value of the bit-reversed circle-domain evaluation), 2^log rows per column.
 *
 * Log sizes: log_plonk = ceil_log2(n_rows) (pad(): next_power_of_two, :283-331); log_poseidon =
 * ceil_log2(6 * max(32, roundup16(n_flow))) with n_flow = the circuit's invocations (copies * flow_count).  The Poseidon
 * rule is not written in the reference (the trace generator sits in the un-vendored stwo fork); it reproduces the header of
 * the next fixture for all 14 consecutive pairs of the reference's fixture chain.  RSV_E_SIZE for zero rows or flow, or
 * a log size beyond RSV_MAX_WITNESS_LOG. */
int rsv_trace_log_sizes(size_t n_rows, size_t n_flow, uint32_t* log_plonk, uint32_t* log_poseidon);
/* The PREPROCESSED columns (host arithmetic, no device), from the unpadded gate list [n_rows][6] and flow wires
 * [n_flow][5] exactly as rsv_witness_program_gates / _export return them.
 *   plonk_pre [10][2^log_plonk]: a_wire, b_wire, c_wire, op, mult_a, mult_b, mult_c, poseidon_wire, mult_poseidon,
 *     enforce_c_m31 (the AIR's order, components/recursive/composition/src/plonk.rs:14-41).  Padding rows (0, 0, 0, op 1);
 *     multiplicities as populate_logup_arguments (:345-466) with num_input = 3 (components/recursive allocates no public
 *     input; the four constant rows the constraint system starts with are checked, RSV_E_RANGE otherwise); 1 - count is
 *     taken mod P.  `op` is the template's: patch the witness_ops rows per proof (rsv_witness_trace_dev's d_ops).
 *   poseidon_pre [40][2^log_poseidon]: is_first, is_last, is_full, round_id, rc0[16], rc1[16], wire of r1 / r3, wire of
 *     r2 / r4, r1 / r3 wire != 0, r2 / r4 wire != 0 (composition/src/poseidon.rs:73-241).  Invocation k (of the flow padded
 *     with wire-0, address-0 entries) sits at rows ((k / 16) * 6 + j) * 16 + k % 16, j < 6; round_id = 6 k + j; rc0[0] of
 *     its first row carries the swap address; rows behind the padded flow have is_first = is_last = 1, all else 0.
 * Log sizes smaller than rsv_trace_log_sizes' (larger is allowed), zero rows or flow: RSV_E_SIZE; NULL: RSV_E_NULL; a
 * Poseidon output wire used more than once: RSV_E_RANGE.  Nothing is written unless RSV_OK. */
int rsv_trace_preprocessed(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, uint32_t log_plonk,
                           uint32_t log_poseidon, uint32_t* plonk_pre, uint32_t* poseidon_pre);
/* The same for a circuit with public inputs: num_input is the reference's, 3 for the constants 1, i, j plus one per
 * new_*(PublicInput); the public inputs are variables 1 .. num_input, each counted once more in the multiplicities.
 * num_input < 3: RSV_E_RANGE.  rsv_trace_preprocessed is this with num_input = 3. */
int rsv_trace_preprocessed_inputs(const uint32_t* gates, size_t n_rows, const uint32_t* flow_wires, size_t n_flow, uint32_t log_plonk,
                                  uint32_t log_poseidon, uint32_t num_input, uint32_t* plonk_pre, uint32_t* poseidon_pre);
/* The TRACE columns of a batch, from what rsv_witness_eval_dev wrote (d_variables in the layout RSV_OPT_WITNESS_LAYOUT
 * names, d_flow / d_flow_swap, d_accept), or from a caller's own (rsv_circuit_program_create).  Programs with a gate list
 * only: built or made from a circuit (RSV_E_SIZE otherwise), as for every later stage; the program's padded wires and
 * witness ops go to the device on the first call.  lp, lq = rsv_trace_log_sizes(gate rows, copies * flow_count).
 *   d_plonk [n][12][2^lp]: a_val, b_val, c_val (4 words each) = variables[wire[row]] (:571-618).
 *   d_poseidon [n][48][2^lq]: in[16], intermediate[16], out[16] of the six rows per invocation above: the state entering
 *     the row's rounds; row 0: intermediate[0] = swap bit, out = external matrix of the (swapped) input; rows 1, 2, 4, 5:
 *     intermediate = the first full round's S-box outputs, out = the state after two full rounds; row 3: intermediate[r] =
 *     the r-th partial S-box output (r < 14).  Invocation k of copy c hashes flow record k - c * flow_count; the padding
 *     invocations hash zeros.  Rows behind the padded flow are zero.
 *   d_ops [n][n_witness_ops]: the `op` of witness-op row k for proof i = variables[bit].x ? constant : 0.
 * Any of the three may be NULL (skipped); d_variables is needed for d_plonk / d_ops, d_flow + d_flow_swap for d_poseidon
 * (RSV_E_NULL otherwise).  d_variables, d_flow, d_poseidon 16-byte aligned.  Every element is written; a proof with
 * d_accept[i] == 0 gets zero columns and zero ops.  Enqueued on the context's stream. */
int rsv_witness_trace_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_variables, const uint32_t* d_flow,
                          const uint8_t* d_flow_swap, const uint8_t* d_accept, size_t n, uint32_t* d_plonk, uint32_t* d_poseidon,
                          uint32_t* d_ops);
/* The same from what rsv_witness_eval_groups_dev wrote, one set of columns per GROUP: d_variables and d_accept of n_groups
 * groups, d_flow [n_groups][copies][flow_count][32] and d_flow_swap [n_groups][copies][flow_count].  Invocation k of copy c
 * hashes flow record k - c * flow_count of the group's proof c.  Outputs, refusals and alignment as rsv_witness_trace_dev
 * with n = n_groups; n_groups * copies <= 2^20.  Every later stage of the chain takes these columns as they are. */
int rsv_witness_trace_groups_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_variables, const uint32_t* d_flow,
                                 const uint8_t* d_flow_swap, const uint8_t* d_accept, size_t n_groups, uint32_t* d_plonk,
                                 uint32_t* d_poseidon, uint32_t* d_ops);
/* rsv_witness_eval + rsv_witness_trace_dev on host buffers (plonk, poseidon, ops may each be NULL). */
int rsv_witness_trace(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                      const rsv_public_input* pi, size_t n_pi, uint32_t* plonk, uint32_t* poseidon, uint32_t* ops, uint8_t* accept,
                      uint8_t* reason, int device);

/* ---- the interaction (logup) columns: tree 2 of the next proof, 8 Plonk + 8 Poseidon ---------------------------------
 * The AIR's relations (components/recursive/composition/src/{data_structures,plonk,poseidon}.rs) add the entries
 * multiplicity / (sum_i alpha^i values[i] - z), batched Plonk {a, b}, {c, poseidon} and Poseidon {in_left, in_right,
 * out_left}, {out_right, swap}; f0, f1 = the two batches' fraction sums at a row.  Per component, two secure columns as
 * 4 M31 coordinate columns each (combine_ef order), rows stored as the trace columns:
 *   columns 0..3: f0 at the row;
 *   columns 4..7: S[k] = sum_{j <= k} (f0[j] + f1[j] - shift) over the domain's COSET order k (the row at position i holds
 *     circle-domain index bitrev(i); coset index 2 d for d < 2^(log-1), 2^(log+1) - 2 d - 1 otherwise), shift = total /
 *     2^log, total = sum over all rows of f0 + f1 = the component's claimed sum (S[last] = 0).
 * For an accepted proof the claimed sums balance the public inputs: plonk + poseidon + sum_(idx, v) 1 / (v + idx alpha - z)
 * = 0, for any (z, alpha).
 *
 * From the trace columns rsv_witness_trace_dev wrote (d_plonk [n][12][2^lp], d_poseidon [n][48][2^lq]), d_accept and the
 * lookup elements the next proof's transcript draws after trees 0 and 1, d_lookup [n][8]: z, then alpha (QM31 words; any
 * u32 is taken mod P).  Programs with a gate list only (built, or made from a circuit: RSV_E_SIZE otherwise); the program's 10 + 40 preprocessed columns, shared with
 * rsv_witness_commit_dev, go to the device on the first call.  Outputs: d_int_plonk [n][8][2^lp], d_int_poseidon
 * [n][8][2^lq], d_sums [n][2][4] (the Plonk then the Poseidon claimed sum), d_ok [n] (may be NULL): 1 iff the proof was
 * accepted and no denominator of either component is zero.  A proof with d_ok[i] == 0 (rejected, or a zero denominator)
 * gets zero columns and zero sums; the other proofs of the batch are unaffected.  Every element is written.  NULL pointers
 * (but d_ok): RSV_E_NULL; d_plonk, d_poseidon, d_lookup, d_sums 4-byte and d_int_plonk, d_int_poseidon 8-byte aligned,
 * RSV_E_SIZE otherwise.  Enqueued on the context's stream; the context's workspace grows (with a synchronisation) only
 * when a batch needs more. */
int rsv_witness_interaction_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                                const uint8_t* d_accept, const uint32_t* d_lookup, size_t n, uint32_t* d_int_plonk,
                                uint32_t* d_int_poseidon, uint32_t* d_sums, uint8_t* d_ok);
/* rsv_witness_eval + rsv_witness_trace_dev + rsv_witness_interaction_dev on host buffers (lookup [n][8]; ok and reason
 * may be NULL). */
int rsv_witness_interaction(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                            const rsv_public_input* pi, size_t n_pi, const uint32_t* lookup, uint32_t* int_plonk, uint32_t* int_poseidon,
                            uint32_t* sums, uint8_t* ok, uint8_t* accept, uint8_t* reason, int device);

/* ---- commitment of a tree of the next proof: interpolation, low-degree extension, Merkle root ------------------------
 * A tree is one or more groups of M31 columns; group g has n_cols columns of 2^log_size rows, stored as the trace columns
 * are (evaluations on CanonicCoset(log_size).circle_domain(), bit-reversed).  Each column is interpolated (CirclePoly
 * coefficients: coefficient i multiplies y^{i_0} x^{i_1} pi(x)^{i_2} pi^2(x)^{i_3} ..., i_k = bit k of i, pi(x) =
 * 2 x^2 - 1), evaluated on CanonicCoset(log_size + log_blowup).circle_domain() (bit-reversed) and the tree is committed
 * with stwo's mixed-size rule: the leaves sit at the largest log_size + log_blowup, leaf = hash_node(None, that layer's
 * columns); a lower layer l is hash_node((L, R), the columns of size 2^l) or just (L, R) where no column has that size.
 * Within a layer the columns go in group order.  hash_node is rsv_merkle_hash_node's.
 *
 * The LDE is streamed in blocks of 2^log_size positions and hashed as it is made: the workspace holds the coefficients, the
 * blocks in flight and the node layers of one pass, within RSV_OPT_WS_BUDGET_MB (a larger batch or tree is cut into passes
 * of fewer blocks, then fewer proofs).  log_size + log_blowup <= RSV_MAX_LOG_SIZE, 1 <= log_blowup <= RSV_MAX_LOG_BLOWUP,
 * 1 <= n_groups <= RSV_MAX_COMMIT_GROUPS, n_cols >= 1, n <= 2^20; RSV_E_SIZE otherwise, and for a pointer that is not
 * 4-byte aligned. */
#define RSV_MAX_COMMIT_GROUPS 8
typedef struct {
    uint32_t log_size;
    uint32_t n_cols;
    const uint32_t* d_cols;  /* [n][n_cols][2^log_size] (device); proof i's columns at d_cols + i * proof_stride */
    uint64_t proof_stride;   /* words between two proofs' column sets; 0: one set shared by every proof */
    uint32_t* d_coeffs;      /* optional output (may be NULL): the coefficients, [n][n_cols][2^log_size] */
    uint32_t* d_lde;         /* optional output (may be NULL): the LDE, [n][n_cols][2^(log_size + log_blowup)], bit-reversed */
} rsv_commit_group;
/* d_roots [n][8] (device).  d_mask [n] (device, may be NULL): a proof whose byte is 0 gets a zero root and zero d_coeffs /
 * d_lde; its neighbours are unaffected.  groups: HOST memory, read during the call.  NULL groups, d_cols or d_roots:
 * RSV_E_NULL.  Enqueued on the context's stream; twiddle tables (one per domain size, kept in the context) and the
 * workspace are allocated, with a synchronisation, only when a call needs more. */
int rsv_commit_tree_dev(rsv_ctx* ctx, const rsv_commit_group* groups, size_t n_groups, size_t n, uint32_t log_blowup,
                        const uint8_t* d_mask, uint32_t* d_roots);

/* rsv_commit_tree_dev that also leaves the tree's CAP: d_cap [n][2^(log_blowup + 1)][8] (device, may be NULL: then exactly
 * rsv_commit_tree_dev), the nodes of layers 0 .. log_blowup in heap order: layer l at entries 2^l .. 2^(l+1) - 1 (entry 1 is
 * the root, entries 2^log_blowup .. are the roots of the streamed blocks' subtrees), entry 0 zero; all zero for a masked
 * proof.  64 B .. 4 MB per proof.  It is what rsv_decommit_tree_dev needs of the tree besides the columns, so a prover
 * pays for the tree once.  The roots are those of rsv_commit_tree_dev, bit for bit.  d_cap 4-byte aligned. */
int rsv_commit_tree_cap_dev(rsv_ctx* ctx, const rsv_commit_group* groups, size_t n_groups, size_t n, uint32_t log_blowup,
                            const uint8_t* d_mask, uint32_t* d_roots, uint32_t* d_cap);

/* ---- decommitment of a tree of the next proof: queried values and Merkle witness --------------------------------------
 * The opening of a tree rsv_commit_tree_dev committed, at a list of positions: what a proof carries for the tree besides
 * its root and sampled values, queried_values[t] and decommitments[t].hash_witness, in stwo's batched order
 * (MerkleProver::decommit; the order SinglePathMerkleProof::from_stwo_proof, components/hints/src/decommit.rs, consumes).
 * The same groups, n, log_blowup and d_mask as the commitment (d_coeffs and d_lde are ignored), plus
 *   d_queries [n][n_queries] (device): positions in the tree's largest layer, top = max(log_size) + log_blowup bits, in
 *     the bit-reversed storage order d_lde is indexed by.  Any order, duplicates allowed; bits above `top` are ignored
 *     (any u32 is taken mod 2^top).  1 <= n_queries <= RSV_MAX_QUERIES.
 *   d_values [n][values_cap], d_n_values [n]: layer by layer from `top` down, for every distinct queried node of the
 *     layer (queries >> (top - layer)) in ascending position, that layer's columns in commitment order (groups of one
 *     size in group order).
 *   d_witness [n][witness_cap][8], d_n_witness [n]: layer by layer from `top` down, for every distinct parent in
 *     ascending order, the child that is not itself on a queried path (none where both are).
 *   The capacities are rsv_decommit_sizes': n_queries * sum(n_cols) words and n_queries * top nodes.  Words past a proof's
 *   count are zero; a masked proof gets zero counts and zero buffers, its neighbours are unaffected.  stwo's
 *   column_witness is always empty for these trees (the smaller columns' queries are the larger ones shifted): there is
 *   no output for it.
 * The tree was streamed and never stored, so the opening recomputes what it opens: the LDE rows and the subtree of a
 * block (position >> (top - log_blowup)) for the values and the witness nodes above layer log_blowup; the witness nodes
 * at layers <= log_blowup come from the tree's cap (rsv_commit_tree_cap_dev).  cap_mode:
 *   RSV_CAP_NONE   no d_cap: every block is recomputed (about one commitment), the cap lives in the workspace;
 *   RSV_CAP_WRITE  the same, and the cap is left in d_cap [n][2^(log_blowup + 1)][8];
 *   RSV_CAP_READ   d_cap is trusted as given and only the blocks the queries touch are recomputed.
 * Refusals as rsv_commit_tree_dev, before any device work: NULL ctx, groups, d_cols, d_queries or an output (d_cap in
 * the modes that use it): RSV_E_NULL; sizes, n_queries, an unknown cap_mode, a pointer not 4-byte aligned: RSV_E_SIZE.
 * Enqueued on the context's stream with no host synchronisation but the workspace's and the twiddle tables' growth; the
 * workspace (the plan, the coefficients, the blocks in flight, two node layers) stays within RSV_OPT_WS_BUDGET_MB by
 * cutting the work into passes of fewer (proof, block) units, as the commitment does. */
enum rsv_cap_mode { RSV_CAP_NONE = 0, RSV_CAP_WRITE = 1, RSV_CAP_READ = 2 };
/* Host arithmetic: the output capacities of rsv_decommit_tree_dev per proof, values in words, witness in nodes. */
int rsv_decommit_sizes(const rsv_commit_group* groups, size_t n_groups, uint32_t log_blowup, uint32_t n_queries, size_t* values_cap,
                       size_t* witness_cap);
int rsv_decommit_tree_dev(rsv_ctx* ctx, const rsv_commit_group* groups, size_t n_groups, size_t n, uint32_t log_blowup,
                          const uint8_t* d_mask, const uint32_t* d_queries, uint32_t n_queries, int cap_mode, uint32_t* d_cap,
                          uint32_t* d_values, uint32_t* d_n_values, uint32_t* d_witness, uint32_t* d_n_witness);

/* Trees 0, 1 and 2 of the recursion circuit's next proof and the transcript between them, from what rsv_witness_trace_dev
 * wrote (d_plonk, d_poseidon, d_ops [n][n_witness_ops]; d_ops may be NULL for a program without witness ops) and d_accept:
 *   tree 0: the program's 10 Plonk + 40 Poseidon preprocessed columns (rsv_trace_preprocessed, uploaded on the first call)
 *           with the op column's witness rows from d_ops;
 *   tree 1: the 12 + 48 trace columns;
 *   then, per proof, the next transcript's prefix: mix root 0, log_size_plonk, log_size_poseidon, root 1, draw (z, alpha);
 *   tree 2: the interaction columns under that (z, alpha) (rsv_witness_interaction_dev, written to d_int_plonk
 *           [n][8][2^lp] and d_int_poseidon [n][8][2^lq], 8-byte aligned; claimed sums to d_sums [n][2][4]);
 *   then mix the two claimed sums and root 2, draw random_coeff.
 * Outputs: d_roots [n][3][8]; d_draws [n][12]: z, alpha, random_coeff (QM31 words); d_channel [n][16] (may be NULL): the
 * channel after the last draw, digest[8] then n_sent then 7 zero words, from which tree 3's stage continues (mix root 3,
 * draw the OODS point); d_ok [n] (may be NULL): 1 iff the proof was accepted and no logup denominator is zero.  A proof
 * with d_ok[i] == 0 gets zeros in every output; the other proofs are unaffected.  1 <= log_blowup <= RSV_MAX_LOG_BLOWUP
 * and max(lp, lq) + log_blowup <= RSV_MAX_LOG_SIZE, else RSV_E_SIZE; alignment as rsv_witness_interaction_dev (d_ops,
 * d_roots, d_draws, d_channel 4 bytes).  Enqueued on the context's stream. */
int rsv_witness_commit_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                           const uint32_t* d_ops, const uint8_t* d_accept, size_t n, uint32_t log_blowup, uint32_t* d_roots,
                           uint32_t* d_draws, uint32_t* d_int_plonk, uint32_t* d_int_poseidon, uint32_t* d_sums, uint32_t* d_channel,
                           uint8_t* d_ok);
/* rsv_witness_commit_dev that also leaves the three trees' caps: d_caps [n][3][2^(log_blowup + 1)][8] (may be NULL: then
 * exactly rsv_witness_commit_dev), each as rsv_commit_tree_cap_dev's; a proof with d_ok[i] == 0 keeps the caps of the
 * trees committed before it was refused, and its roots are zero. */
int rsv_witness_commit_caps_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                                const uint32_t* d_ops, const uint8_t* d_accept, size_t n, uint32_t log_blowup, uint32_t* d_roots,
                                uint32_t* d_draws, uint32_t* d_int_plonk, uint32_t* d_int_poseidon, uint32_t* d_sums,
                                uint32_t* d_channel, uint8_t* d_ok, uint32_t* d_caps);
/* The decommitment of trees 0, 1 and 2 of the recursion circuit's next proof (rsv_decommit_tree_dev three times, on the
 * trees rsv_witness_commit_dev commits) from the buffers the chain holds: d_plonk, d_poseidon, d_ops, the interaction
 * columns d_int_plonk and d_int_poseidon, and the mask d_ok (rsv_witness_commit_dev's; NULL: d_accept is the mask).
 * d_queries [n][n_queries] at the trees' own largest layer, max(lp, lq) + log_blowup bits.  d_caps [n][3][2^(log_blowup +
 * 1)][8] from rsv_witness_commit_caps_dev (RSV_CAP_READ), or NULL (RSV_CAP_NONE).  Outputs, with tree t's capacities
 * v_t, w from rsv_decommit_sizes (groups (lp, 10), (lq, 40); (lp, 12), (lq, 48); (lp, 8), (lq, 8)): d_values
 * [n][v_0 + v_1 + v_2] (a proof's three trees one after the other), d_n_values [n][3], d_witness [n][3][w][8],
 * d_n_witness [n][3].  Programs with a gate list only (built, or made from a circuit); refusals and alignment as rsv_witness_commit_dev and rsv_decommit_tree_dev. */
int rsv_witness_decommit_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                             const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon,
                             const uint8_t* d_accept, const uint8_t* d_ok, size_t n, uint32_t log_blowup, const uint32_t* d_queries,
                             uint32_t n_queries, const uint32_t* d_caps, uint32_t* d_values, uint32_t* d_n_values,
                             uint32_t* d_witness, uint32_t* d_n_witness);
/* rsv_witness_eval + rsv_witness_trace_dev + rsv_witness_commit_dev on host buffers: roots [n][3][8], draws [n][12], sums
 * [n][2][4] (ok and reason may be NULL). */
int rsv_witness_commit(const rsv_witness_program* prog, const uint8_t* blob, const uint64_t* offsets, size_t n, const rsv_cfg_set* cfg,
                       const rsv_public_input* pi, size_t n_pi, uint32_t log_blowup, uint32_t* roots, uint32_t* draws, uint32_t* sums,
                       uint8_t* ok, uint8_t* accept, uint8_t* reason, int device);

/* ---- sampled values of a tree of the next proof: the columns at the OODS point ----------------------------------------
 * What a proof carries for a tree besides its root and its opening: sampled_values[t], the value of every column's
 * interpolant (CirclePoly::eval_at_point of the coefficients rsv_commit_group::d_coeffs documents) at QM31 points.  The
 * same groups, n and d_mask as rsv_commit_tree_dev (d_coeffs and d_lde are ignored), plus
 *   source    RSV_SAMPLE_COLUMNS: d_cols holds the evaluations, as for the commitment; they are interpolated in the
 *             workspace by the commitment's own interpolation, in passes of fewer proofs under RSV_OPT_WS_BUDGET_MB.
 *             RSV_SAMPLE_COEFFS: d_cols holds what a commitment wrote to d_coeffs; the workspace is the weight tables
 *             and partial sums alone.  The words must be canonical (< P), as a commitment's are: unlike the point
 *             words they are NOT reduced, and a word >= P is not refused either: the values of that column are then
 *             unspecified (the unreduced 64-bit sums may wrap), those of the other columns unaffected.
 *   d_points  [n][n_points][8] (device): per proof and point x then y, QM31 words; any u32 is taken mod P.  The point
 *             need not lie on the circle.  1 <= n_points <= RSV_MAX_SAMPLE_POINTS.
 *   d_samples [n][n_points][sum n_cols][4] (device): the columns in group order.  Every element is written; zeros for a
 *             masked proof, its neighbours unaffected.
 * log_size <= RSV_MAX_LOG_SIZE - 1 (log_size 0: the constant).  Refusals before any device work: NULL ctx, groups,
 * d_cols, d_points or d_samples: RSV_E_NULL; group sizes, n, n_points, an unknown source, a pointer not 4-byte aligned:
 * RSV_E_SIZE.  Enqueued on the context's stream with no host synchronisation but the workspace's and the twiddle
 * tables' growth. */
#define RSV_MAX_SAMPLE_POINTS 4
enum rsv_sample_source { RSV_SAMPLE_COLUMNS = 0, RSV_SAMPLE_COEFFS = 1 };
int rsv_sample_tree_dev(rsv_ctx* ctx, const rsv_commit_group* groups, size_t n_groups, size_t n, const uint8_t* d_mask, int source,
                        const uint32_t* d_points, uint32_t n_points, uint32_t* d_samples);
/* sampled_values[0..2] of the recursion circuit's next proof from the buffers the chain holds (arguments as
 * rsv_witness_decommit_dev's leading ones; the mask is d_ok, or d_accept when d_ok is NULL) and the OODS point d_oods
 * [n][8] (x then y; any u32 is taken mod P).  d_samples [n][134][4] in the proof's own order, tree-major, column-major,
 * sample-minor: tree 0 at values 0..49 and tree 1 at 50..109, one value per column at the OODS point; tree 2 at
 * 110..133, per component columns 0..3 one value and the cumulative columns 4..7 two, first at the previous-row point
 * (the OODS point minus the step of CanonicCoset(the component's log size), formed on the device), then at the OODS
 * point.  Zeros for a masked proof.  Programs with a gate list only (built, or made from a circuit); refusals and alignment as rsv_witness_decommit_dev. */
int rsv_witness_sample_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                           const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon,
                           const uint8_t* d_accept, const uint8_t* d_ok, size_t n, const uint32_t* d_oods, uint32_t* d_samples);

/* ---- tree 3 of the next proof: the composition polynomial -------------------------------------------------------------
 * With clb = max(lp + 2, lq + 3) (the verifier's composition log degree bound) and L3 = clb - 1: for a point p of
 * CanonicCoset(clb).circle_domain(), A(p) is the accumulator of CompositionCheck::compute over the 86 constraints (6 Plonk,
 * then 80 Poseidon): acc = acc * random_coeff + constraint / Z_l(p), Z_l(p) = pi^(l-1)(p.x) for the component's log size l,
 * the mask values being the 126 columns' interpolants at p (the cumulative interaction columns 4..7 of each component
 * also at p minus the step of CanonicCoset(l)) and the claimed-sum shift sum / 2^l.  The four QM31 coordinates of A on the
 * 2^clb positions (bit-reversed) are interpolated as columns are (rsv_commit_group::d_coeffs' convention) and the
 * coefficients cut at the middle: C = left + pi^(clb-2)(x) * right.  Tree 3 has eight columns of 2^L3 rows, stored as the
 * trace columns are: column k is coordinate k of left, column 4 + k coordinate k of right.  The definition is exact for
 * arbitrary columns, not only satisfying ones.
 * rsv_composition_log_size: host arithmetic, L3 for (lp, lq); RSV_E_SIZE for sizes rsv_composition_dev refuses. */
int rsv_composition_log_size(uint32_t lp, uint32_t lq, uint32_t* log_size);
/* The generic call on raw device columns: the Plonk component's preprocessed [10][2^lp], trace [n][12][2^lp] and
 * interaction [n][8][2^lp] columns, the Poseidon component's [40], [48], [8] at 2^lq, each with its proof stride in words
 * (0: one set shared by every proof, as rsv_commit_group::proof_stride); d_sums [n][2][4] and d_draws [n][12] (z, alpha,
 * random_coeff) as rsv_witness_commit_dev leaves them (any u32 is taken mod P); d_mask [n] (may be NULL).  Outputs: d_comp
 * [n][8][2^L3], the form rsv_commit_tree_dev takes, and d_comp_coeffs (may be NULL) of the same shape, the columns'
 * coefficients (left and right themselves), the form RSV_SAMPLE_COEFFS takes.  Every element is written; a masked proof
 * gets zeros, its neighbours are unaffected.  The columns are extended to 2^clb rows by the commitment's interpolation
 * and forward FFT, in aligned blocks of rows within RSV_OPT_WS_BUDGET_MB (fewer blocks, then fewer proofs; the
 * accumulator's 4 x 2^clb words per proof stay in the workspace).  Refusals before any device work: a NULL pointer (but
 * d_mask, d_comp_coeffs): RSV_E_NULL; lp or lq below 2, clb above RSV_MAX_LOG_SIZE, n above 2^20, a pointer not 4-byte
 * aligned: RSV_E_SIZE.  Enqueued on the context's stream with no host synchronisation but the workspace's and the
 * twiddle tables' growth. */
int rsv_composition_dev(rsv_ctx* ctx, uint32_t lp, uint32_t lq, const uint32_t* d_plonk_pre, uint64_t plonk_pre_stride,
                        const uint32_t* d_plonk, uint64_t plonk_stride, const uint32_t* d_int_plonk, uint64_t int_plonk_stride,
                        const uint32_t* d_poseidon_pre, uint64_t poseidon_pre_stride, const uint32_t* d_poseidon,
                        uint64_t poseidon_stride, const uint32_t* d_int_poseidon, uint64_t int_poseidon_stride, const uint32_t* d_sums,
                        const uint32_t* d_draws, const uint8_t* d_mask, size_t n, uint32_t* d_comp, uint32_t* d_comp_coeffs);
/* Tree 3 of the recursion circuit's next proof from the buffers the chain holds (leading arguments as
 * rsv_witness_sample_dev's; the mask is d_ok, or d_accept when d_ok is NULL) and what rsv_witness_commit_dev left in
 * d_sums, d_draws and d_channel [n][16] (read and updated):
 *   the composition columns d_comp [n][8][2^L3], which the caller keeps for a later rsv_decommit_tree_dev;
 *   their commitment, one group (L3, 8), as rsv_commit_tree_cap_dev: d_root3 [n][8], d_cap3 [n][2^(log_blowup + 1)][8]
 *   (may be NULL);
 *   per proof, mix root 3 and draw t: the OODS point ((1 - t^2) / (1 + t^2), 2 t / (1 + t^2)) to d_oods [n][8], x then y,
 *   the form rsv_witness_sample_dev takes, and the channel after the draw to d_channel;
 *   d_samples3 [n][8][4]: the eight columns at that point (sampled_values[3]).
 * A proof whose mask byte is 0 gets zeros in every output; its neighbours are unaffected.  Programs with a gate list only (built, or made from a circuit).  Refusals
 * as rsv_witness_sample_dev and rsv_composition_dev; L3 + log_blowup above RSV_MAX_LOG_SIZE or log_blowup outside
 * 1 .. RSV_MAX_LOG_BLOWUP: RSV_E_SIZE. */
int rsv_witness_tree3_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                          const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept,
                          const uint8_t* d_ok, size_t n, uint32_t log_blowup, const uint32_t* d_sums, const uint32_t* d_draws,
                          uint32_t* d_channel, uint32_t* d_comp, uint32_t* d_root3, uint32_t* d_cap3, uint32_t* d_oods,
                          uint32_t* d_samples3);

/* ---- the commit phase of FRI of the next proof: DEEP quotients, layer trees, folds, the last polynomial -------------------
 * The definition is the verifier's (rsv_verify_batch_dev forms the same quotients and folds per query), evaluated at every
 * position.  Sizes below are LDE log sizes: a column group of log size l gives values on
 * CanonicCoset(l + log_blowup).circle_domain(), bit-reversed.
 * Quotients: the groups of one log size form one QM31 quotient column, their columns in group order.  Sample k of a column
 * (value v at the point (px, py)) has the line coefficients a = w v.b, b = w (v.a py.b - v.b py.a), c = w py.b (v = (v.a,
 * v.b) in CM31 halves), w the running power of `after`: -2u at the column's first sample, then times `after` per sample
 * through batch 0 (the samples at point 0, in column order), batch 1, ...  At position q with domain point (x, y):
 *   value = sum over batches of (sum_k c_k row[col_k] - (a_k y + b_k)) / ((px.a - x) py.b - (py.a - y) px.b).
 * Folds: pair (2k, 2k + 1) of a column of size l gives (f0 + f1) + alpha[M - l] (f0 - f1) / y, y of the pair's first point
 * (circle to line), of a line layer of size l (f0 + f1) + alpha (f0 - f1) / x, x of half_odds(l).at(bit_reverse(2k, l)).
 * With M the largest size: the first tree commits every column (four M31 coordinate columns each) by rsv_commit_tree_dev's
 * mixed-size rule; the running line evaluation starts as the size-M column's fold (log size M - 1); inner layer i is the
 * evaluation at log size M - 1 - i, committed as a four-column tree, folded under alpha[i + 1] to log size M - 2 - i, after
 * which a column of size M - 1 - i joins: evaluation * alpha[i + 1]^2 + the column's fold under alpha[i + 1].  n_inner =
 * M - 1 - log_last - log_blowup layers leave 2^(log_last + log_blowup) values, whose line-polynomial coefficients in
 * degree order are cut at 2^log_last: the first 2^log_last are the last layer's polynomial, stored in the bit-reversed
 * order rsv_line_eval reads; the rest are zero exactly when the input was of low degree.
 * Transcript: mix the first root, draw alpha[0]; per inner layer mix its root, draw alpha[i + 1]; mix the last
 * polynomial's coefficients two per mix (a single one at the end of an odd count).
 *
 * rsv_fri_sizes: host arithmetic for the recursion circuit's shape (log sizes lp, lq): sizes[3] the distinct quotient
 * sizes descending (lde of tree 3: max(lp + 1, lq + 2) + log_blowup, then lp + log_blowup and lq + log_blowup), their
 * number, n_inner, and the words per proof of d_quot, d_layers and d_last_poly.  RSV_E_SIZE for what rsv_witness_fri_dev
 * refuses of the sizes, but for one case: min(lp, lq) == log_last + 1 is answered here and refused by rsv_witness_fri_dev
 * (RSV_E_SIZE) — the smallest column would enter the fold behind the last inner layer, where the reference's prover
 * asserts and no verifier folds it in (the proof would be RSV_R_FRI_LAST); rsv_fri_commit_dev, which serves no verifier,
 * takes such sizes. */
int rsv_fri_sizes(uint32_t lp, uint32_t lq, uint32_t log_blowup, uint32_t log_last, uint32_t* sizes, uint32_t* n_sizes, uint32_t* n_inner,
                  size_t* quot_words, size_t* layer_words, size_t* last_words);
/* Which points apply to a group's columns: point k (< n_points) to the columns col_lo[k] .. col_hi[k] - 1 (col_hi[k] <=
 * col_lo[k]: to none).  Host memory. */
typedef struct rsv_fri_group_points {
    uint32_t col_lo[4]; /* RSV_MAX_SAMPLE_POINTS */
    uint32_t col_hi[4];
} rsv_fri_group_points;
/* The quotient columns of column groups (rsv_commit_group: log_size, n_cols, d_cols, proof_stride; d_coeffs and d_lde are
 * not used), 1 <= log_size, log_size + log_blowup <= RSV_MAX_LOG_SIZE.
 *   source        as rsv_sample_tree_dev: RSV_SAMPLE_COLUMNS (d_cols holds evaluations) or RSV_SAMPLE_COEFFS (canonical
 *                 coefficients, as a commitment's d_coeffs).
 *   d_points      [n][n_points][8]: x then y; any u32 is taken mod P.  Batches are taken in ascending point index.
 *   d_samples     [n][n_points][sum n_cols][4], the layout rsv_sample_tree_dev writes for these groups and points; only
 *                 the values group_points selects are read.
 *   d_after       [n][4]: the random coefficient.
 *   d_quot        per proof the columns in descending size, each [4][2^(log_size + log_blowup)] coordinate-major, the form
 *                 a column group has.  Every element is written; zeros for a masked proof (d_mask [n], may be NULL).
 * The extended rows never exist whole: each column's groups are interpolated and extended block by block within
 * RSV_OPT_WS_BUDGET_MB (fewer blocks, then fewer proofs).  Refusals before any device work: a NULL pointer (but d_mask):
 * RSV_E_NULL; n_groups, n_points, log_blowup, sizes, col_hi above n_cols, n above 2^20, an unknown source, a pointer not
 * 4-byte aligned: RSV_E_SIZE.  Enqueued on the context's stream with no host synchronisation but the workspace's and the
 * twiddle tables' growth. */
int rsv_fri_quotients_dev(rsv_ctx* ctx, const rsv_commit_group* groups, const rsv_fri_group_points* group_points, size_t n_groups, size_t n,
                          uint32_t log_blowup, const uint8_t* d_mask, int source, const uint32_t* d_points, uint32_t n_points,
                          const uint32_t* d_samples, const uint32_t* d_after, uint32_t* d_quot);
/* The layers of d_quot (sizes [n_sizes], HOST: the columns' LDE log sizes, strictly descending): d_channel [n][16] read
 * and updated (the state after the last mix is what the proof-of-work stage continues from); d_roots [n][1 + n_inner][8];
 * d_alphas [n][1 + n_inner][4]; d_layers per proof the inner layers' evaluations one after another, layer i
 * [4][2^(M - 1 - i)] (may be NULL when n_inner is 0); d_last_poly [n][2^log_last][4]; d_low_degree [n] bytes: 1 iff every
 * coefficient past 2^log_last is zero.  A masked proof gets zeros in every output and a zeroed channel.  Proofs in passes
 * within RSV_OPT_WS_BUDGET_MB.  Refusals before any device work: a NULL pointer (but d_mask): RSV_E_NULL; n_sizes 0 or
 * above RSV_MAX_COMMIT_GROUPS, sizes not descending or above RSV_MAX_LOG_SIZE, a column of log size (size - log_blowup)
 * <= log_last, log_last > RSV_MAX_LOG_LAST_LAYER, n_inner > RSV_MAX_FRI_INNER, log_blowup outside 1 .. RSV_MAX_LOG_BLOWUP,
 * n above 2^20, a pointer not 4-byte aligned: RSV_E_SIZE. */
int rsv_fri_commit_dev(rsv_ctx* ctx, const uint32_t* d_quot, const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup, uint32_t log_last,
                       size_t n, const uint8_t* d_mask, uint32_t* d_channel, uint32_t* d_roots, uint32_t* d_alphas, uint32_t* d_layers,
                       uint32_t* d_last_poly, uint8_t* d_low_degree);
/* The commit phase of FRI of the recursion circuit's next proof from the buffers the chain holds (leading arguments as
 * rsv_witness_tree3_dev's; the mask is d_ok, or d_accept when d_ok is NULL): d_comp, d_oods and d_samples3 [n][8][4] as
 * rsv_witness_tree3_dev left them, d_samples [n][134][4] as rsv_witness_sample_dev, d_channel [n][16] (read and updated).
 * Per proof: mix the 142 sampled values two per mix, draw `after` (to d_after [n][4]); the quotient columns d_quot (sizes
 * and words: rsv_fri_sizes) from tree 3's columns at the OODS point, and per tree 0, 1, 2 the Plonk and the Poseidon
 * columns at the OODS point and then the cumulative interaction columns 4..7 at the previous-row points (formed on the
 * device); then rsv_fri_commit_dev's outputs.  d_quot and d_layers stay with the caller for the openings.  A masked proof
 * gets zeros in every output and a zeroed channel.  Programs with a gate list only (built, or made from a circuit).  Refusals as rsv_witness_tree3_dev and
 * rsv_fri_commit_dev. */
int rsv_witness_fri_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                        const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept,
                        const uint8_t* d_ok, size_t n, uint32_t log_blowup, uint32_t log_last, const uint32_t* d_comp,
                        const uint32_t* d_oods, const uint32_t* d_samples, const uint32_t* d_samples3, uint32_t* d_channel,
                        uint32_t* d_after, uint32_t* d_quot, uint32_t* d_roots, uint32_t* d_alphas, uint32_t* d_layers,
                        uint32_t* d_last_poly, uint8_t* d_low_degree);

/* ---- proof of work and queries of the next proof -------------------------------------------------------------------------
 * The definition is the verifier's (rsv_verify_batch_dev checks the same mix and draws the same positions).  A nonce is
 * mixed as the QM31 (w0, w1, w2, 0): w0 = nonce & (2^22 - 1), w1 = (nonce >> 22) & (2^21 - 1), w2 = (nonce >> 43) &
 * (2^21 - 1) — one permutation of (w0, w1, w2, 0, 0, 0, 0, 0 || digest), whose capacity half is the new digest; it
 * qualifies when the canonical digest word 0 has pow_bits low zero bits.  The queries are the words of the draws that
 * follow (n_sent restarts at 0 after the mix): ceil(n_queries / 8) draws of eight words each, in order, each word cut
 * to its low log_size bits; the recursion circuit's surplus draws are not made.
 *
 * rsv_pow_grind_dev: the smallest nonce >= start whose mix leaves pow_bits low zero bits in digest word 0 (the
 * reference's grinder starts at 0), among the max_tries candidates start .. start + max_tries - 1 (max_tries 0: 2^(pow_bits
 * + 6), with which a search fails with probability about e^-64).
 *   d_channel   [n][16] in the form rsv_witness_fri_dev leaves: digest, n_sent, seven zero words.  Read and updated: the
 *               nonce is mixed in.
 *   d_nonce     [n][2], low word first.
 *   d_ok        [n] bytes, required: read as the mask, and cleared for a proof whose search is exhausted.
 * A masked or exhausted proof gets a zero nonce and a zeroed channel; its neighbours are unaffected.  One lane per
 * candidate; a lane that finds a qualifying nonce lowers the proof's minimum, every lane leaves at the first of its
 * candidates that is not below that minimum.  Refusals before any device work: a NULL pointer: RSV_E_NULL; pow_bits >
 * RSV_MAX_POW_BITS, n 0 or above 2^20, start + max_tries overflowing 64 bits, a pointer not 4-byte aligned: RSV_E_SIZE.
 * Enqueued on the context's stream with no host synchronisation but the workspace's growth. */
int rsv_pow_grind_dev(rsv_ctx* ctx, uint32_t pow_bits, uint64_t start, uint64_t max_tries, size_t n, uint8_t* d_ok, uint32_t* d_channel,
                      uint32_t* d_nonce);
/* The query positions: d_channel [n][16] as rsv_pow_grind_dev left it (read and updated: n_sent moves on by the draws);
 * d_queries [n][n_queries], positions of log_size bits in draw order, unsorted and with duplicates kept — what
 * rsv_decommit_tree_dev takes; d_queries_low (may be NULL) [n][n_queries]: the same positions >> (log_size - log_size_low),
 * for the trees whose largest layer is smaller.  1 <= n_queries <= RSV_MAX_QUERIES, 1 <= log_size_low <= log_size <=
 * RSV_MAX_LOG_SIZE.  A masked proof (d_mask [n], may be NULL) gets zero positions and a zeroed channel.  Refusals before any
 * device work: a NULL pointer (but d_mask, d_queries_low): RSV_E_NULL; n 0 or above 2^20, the limits above, a pointer not
 * 4-byte aligned: RSV_E_SIZE.  Enqueued on the context's stream with no host synchronisation. */
int rsv_draw_queries_dev(rsv_ctx* ctx, size_t n, const uint8_t* d_mask, uint32_t n_queries, uint32_t log_size, uint32_t log_size_low,
                         uint32_t* d_channel, uint32_t* d_queries, uint32_t* d_queries_low);

/* ---- the openings of the FRI layer trees of the next proof ------------------------------------------------------------------
 * stwo's pair-tree decommitment, as SinglePairMerkleProof::from_stwo_proof consumes it.  Tree 0 is the first layer (leaves
 * at M = sizes[0], a QM31 value per node at every layer in sizes), tree 1 + i inner layer i (leaves at M - 1 - i, values
 * there only); T = 1 + n_inner trees per proof.  For a tree with leaves at `top` and values at the layers D, Q_l the distinct
 * (query >> (top - l)) ascending, S_l = Q_l and their siblings (x ^ 1) for l in D and Q_l elsewhere:
 *   fri_witness   for l in D descending, the value (four words) at every x in S_l ascending that is not in Q_l;
 *   hash_witness  for l = top - 1 .. 0 and x in S_l ascending, the nodes 2x and then 2x + 1 of layer l + 1 that are not in
 *                 S_(l+1): a sibling nobody queries at a lower data layer gives both its children.
 *
 * rsv_fri_open_sizes: the capacities per (proof, tree), host arithmetic: values_cap = n_sizes * n_queries values,
 * witness_cap = n_queries * (M + 2 * (n_sizes - 1)) nodes.  Both are bounds (a level without values gives at most n_queries
 * nodes, a level with values below the top at most 3 n_queries), not tight.  Refusals as rsv_fri_open_dev's. */
int rsv_fri_open_sizes(const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup, uint32_t log_last, uint32_t n_queries, size_t* values_cap,
                       size_t* witness_cap);
/* d_quot, sizes [n_sizes] (HOST) and d_layers exactly as rsv_fri_commit_dev takes and leaves them (d_layers may be NULL only
 * when n_inner is 0); d_queries [n][n_queries] positions of M bits as rsv_draw_queries_dev writes them: any order,
 * duplicates allowed, bits above M ignored (rsv_decommit_tree_dev's contract; inner layer i is opened at query >> (1 + i)).
 *   d_fri_witness    [n][T][values_cap][4],  d_n_fri_witness  [n][T] values;
 *   d_hash_witness   [n][T][witness_cap][8], d_n_hash_witness [n][T] nodes.
 * Every word is written, zero past a count; a masked proof (d_mask [n], may be NULL) gets zero counts and zero buffers.
 * The recompute form: rsv_fri_commit_dev keeps the roots only, so every tree is hashed again by the commitment's own
 * kernel, level by level through two node buffers, and the planned nodes are copied out while their level is there — an
 * opening costs about the layer trees of a commitment.  Proofs in passes within RSV_OPT_WS_BUDGET_MB.  Refusals before any
 * device work: a NULL pointer (but d_mask and d_layers): RSV_E_NULL; what rsv_fri_commit_dev refuses of sizes, log_blowup,
 * log_last and n: RSV_E_SIZE; then, n_inner being known only from sound sizes, a NULL d_layers with n_inner > 0: RSV_E_NULL;
 * n_queries outside 1 .. RSV_MAX_QUERIES, a pointer not 4-byte aligned: RSV_E_SIZE.
 * Enqueued on the context's stream with no host synchronisation but the workspace's growth. */
int rsv_fri_open_dev(rsv_ctx* ctx, const uint32_t* d_quot, const uint32_t* d_layers, const uint32_t* sizes, size_t n_sizes,
                     uint32_t log_blowup, uint32_t log_last, size_t n, const uint8_t* d_mask, const uint32_t* d_queries,
                     uint32_t n_queries, uint32_t* d_fri_witness, uint32_t* d_n_fri_witness, uint32_t* d_hash_witness,
                     uint32_t* d_n_hash_witness);

/* ---- the caps of the FRI layer trees --------------------------------------------------------------------------------------
 * The commitment keeps the top of every layer tree; the opening then hashes only the subtrees that hold a witness node.
 * sub_log = h, 1 <= h <= RSV_MAX_FRI_SUB_LOG.  A tree with leaves at `top` keeps its layers 1 .. c, c = max(top - h, 0) (the
 * root, layer 0, is in d_roots and nobody's witness; a tree with top <= h keeps nothing); below layer c it is 2^c subtrees of
 * 2^(top - c) leaves.  d_caps is level-major and proof-minor: tree after tree (t = 0 .. n_inner), within a tree layer 1 .. c_t
 * one after another, a layer [n][2^l][8] — the form the commitment's level kernel writes and reads, so the kept levels are
 * written where they stay and the commitment gains no launch.  Tree t begins tree_words[t] words into d_caps, its layer l
 * n * 8 * (2^l - 2) words after that, proof p's nodes of it p * 8 * 2^l words further.
 *
 * rsv_fri_cap_sizes: host arithmetic: cap_words = n * sum over the trees of 8 * (2^(c_t + 1) - 2), the words of d_caps for n
 * proofs, and tree_words [1 + n_inner] (may be NULL).  Refusals as rsv_fri_open_sizes' (n above 2^20 with them); sub_log
 * outside 1 .. RSV_MAX_FRI_SUB_LOG: RSV_E_SIZE. */
#define RSV_MAX_FRI_SUB_LOG 8
int rsv_fri_cap_sizes(const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup, uint32_t log_last, uint32_t sub_log, size_t n,
                      size_t* cap_words, size_t* tree_words);
/* rsv_fri_commit_dev that also leaves d_caps [cap_words]; with d_caps NULL it is exactly rsv_fri_commit_dev (sub_log is not
 * read).  Every other output is bit for bit rsv_fri_commit_dev's, through the same launches.  Every word of d_caps is
 * written, pass by pass where the proofs are cut into passes; a masked proof's entries are defined but meaningless.
 * Refusals before any device work: rsv_fri_commit_dev's, in its order; sub_log outside 1 .. RSV_MAX_FRI_SUB_LOG, d_caps not
 * 4-byte aligned: RSV_E_SIZE. */
int rsv_fri_commit_cap_dev(rsv_ctx* ctx, const uint32_t* d_quot, const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup,
                           uint32_t log_last, size_t n, const uint8_t* d_mask, uint32_t* d_channel, uint32_t* d_roots, uint32_t* d_alphas,
                           uint32_t* d_layers, uint32_t* d_last_poly, uint8_t* d_low_degree, uint32_t sub_log, uint32_t* d_caps);
/* rsv_witness_fri_dev with the same two trailing arguments (sizes for rsv_fri_cap_sizes: rsv_fri_sizes'); d_caps NULL:
 * exactly rsv_witness_fri_dev. */
int rsv_witness_fri_caps_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                             const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept,
                             const uint8_t* d_ok, size_t n, uint32_t log_blowup, uint32_t log_last, const uint32_t* d_comp,
                             const uint32_t* d_oods, const uint32_t* d_samples, const uint32_t* d_samples3, uint32_t* d_channel,
                             uint32_t* d_after, uint32_t* d_quot, uint32_t* d_roots, uint32_t* d_alphas, uint32_t* d_layers,
                             uint32_t* d_last_poly, uint8_t* d_low_degree, uint32_t sub_log, uint32_t* d_caps);
/* ---- the tail form of the commit phase --------------------------------------------------------------------------------------
 * rsv_fri_commit_cap_dev with one more argument, tail_log = t, 0 <= t <= RSV_MAX_FRI_TAIL_LOG.  t = 0 is exactly
 * rsv_fri_commit_cap_dev (d_caps NULL: rsv_fri_commit_dev, sub_log is not read): one launch per tree level, one channel launch
 * and one or two fold launches per layer.  With t > 0 every output, d_caps included, is bit for bit the same, through fewer
 * launches: the levels t .. 0 of every layer tree and the channel step on its root are one launch, a workgroup per proof that
 * hashes them in LDS (a tree with leaves at or below level t entirely); and, when log_last + log_blowup <= t, every inner
 * layer of log size <= t (its tree, its channel step, its fold and the column that joins it) and the last layer (the
 * interpolation, d_last_poly, d_low_degree, the final mixes) are one launch more, a workgroup per proof with the evaluation
 * kept in LDS (64 KiB at t = 10).  It pays for one proof, and at t up to about 8: a level of more than 256 nodes takes the one
 * workgroup several rounds of dependent permutations where the per-layer form spreads it over as many compute units, and
 * those rounds, not the launch boundaries, are what the commit phase costs (profiles/HISTORY.md, "FRI tail").
 * Refusals before any device work: rsv_fri_commit_cap_dev's, in its order; then tail_log > RSV_MAX_FRI_TAIL_LOG: RSV_E_SIZE. */
#define RSV_MAX_FRI_TAIL_LOG 10
int rsv_fri_commit_tail_dev(rsv_ctx* ctx, const uint32_t* d_quot, const uint32_t* sizes, size_t n_sizes, uint32_t log_blowup,
                            uint32_t log_last, size_t n, const uint8_t* d_mask, uint32_t* d_channel, uint32_t* d_roots, uint32_t* d_alphas,
                            uint32_t* d_layers, uint32_t* d_last_poly, uint8_t* d_low_degree, uint32_t sub_log, uint32_t* d_caps,
                            uint32_t tail_log);
/* rsv_witness_fri_caps_dev with the same trailing argument; tail_log 0: exactly rsv_witness_fri_caps_dev.  Refusals: its own,
 * in its order; then tail_log > RSV_MAX_FRI_TAIL_LOG: RSV_E_SIZE. */
int rsv_witness_fri_tail_dev(rsv_ctx* ctx, const rsv_witness_program* prog, const uint32_t* d_plonk, const uint32_t* d_poseidon,
                             const uint32_t* d_ops, const uint32_t* d_int_plonk, const uint32_t* d_int_poseidon, const uint8_t* d_accept,
                             const uint8_t* d_ok, size_t n, uint32_t log_blowup, uint32_t log_last, const uint32_t* d_comp,
                             const uint32_t* d_oods, const uint32_t* d_samples, const uint32_t* d_samples3, uint32_t* d_channel,
                             uint32_t* d_after, uint32_t* d_quot, uint32_t* d_roots, uint32_t* d_alphas, uint32_t* d_layers,
                             uint32_t* d_last_poly, uint8_t* d_low_degree, uint32_t sub_log, uint32_t* d_caps, uint32_t tail_log);
/* rsv_fri_open_dev from the caps: outputs and capacities are rsv_fri_open_dev's, word for word; every word is written, zero
 * past a count, zeros for a masked proof (whose entries of d_caps are never read).  d_caps is trusted as given (as a cap
 * under RSV_CAP_READ), with the sub_log and n it was written with.  A witness node at a layer <= c is read from d_caps; one
 * above layer c comes from the subtree under its layer-c ancestor, which one workgroup hashes again in LDS from d_quot /
 * d_layers: at most 2 n_queries subtrees per (proof, tree), six launches whatever M is, no node buffers in the workspace.
 * Refusals before any device work: rsv_fri_open_dev's, in its order, d_caps NULL among the pointers (RSV_E_NULL), sub_log
 * outside 1 .. RSV_MAX_FRI_SUB_LOG with n_queries and d_caps not 4-byte aligned with the pointers (RSV_E_SIZE). */
int rsv_fri_open_cap_dev(rsv_ctx* ctx, const uint32_t* d_quot, const uint32_t* d_layers, const uint32_t* sizes, size_t n_sizes,
                         uint32_t log_blowup, uint32_t log_last, size_t n, const uint8_t* d_mask, const uint32_t* d_queries,
                         uint32_t n_queries, uint32_t* d_fri_witness, uint32_t* d_n_fri_witness, uint32_t* d_hash_witness,
                         uint32_t* d_n_hash_witness, uint32_t sub_log, const uint32_t* d_caps);

/* ---- the next proof serialised: the chain's buffers into the verifier's blob layout ------------------------------------------
 * What the stages above leave, put into the bytes of a PlonkWithPoseidonProof on the device: n proofs as (d_blob,
 * d_offsets), the pair every _dev entry point that takes a blob consumes (rsv_verify_batch_dev, rsv_witness_eval_dev of the
 * next recursion level).  The bytes (bincode: little-endian 32-bit words, every length prefix a u64 = two
 * words, low first; every column_witness empty), T = n_layers = 1 + n_inner:
 *   head, 895 words     log_size_plonk, log_size_poseidon; the eight words of d_sums; pow_bits, log_blowup, log_last;
 *                       u64(n_queries); u64(4) and the four commitments (d_roots' three, d_root3); u64(4) and per tree
 *                       u64(columns) (50, 60, 16, 8), per column u64(samples) and its samples of four words: one per column,
 *                       in tree 2 two for columns 4 .. 7 and 12 .. 15 — d_samples' 134 in order, then d_samples3's eight;
 *   decommitments       u64(4); per tree 0 .. 3: u64(count), the hash_witness nodes of eight words, u64(0) (column_witness);
 *   queried_values      u64(4); per tree 0 .. 3: u64(count), the values of one word;
 *   proof of work       d_nonce's two words;
 *   first layer         u64(count), the fri_witness values of four words; u64(count), the hash_witness nodes; u64(0)
 *                       (column_witness); the eight words of d_fri_roots[0];
 *   inner layers        u64(T - 1) (u64(0) when T is 1), then T - 1 layers in the first layer's form, trees 1 .. T - 1;
 *   last layer          u64(2^log_last), d_last_poly's values of four words; the word log_last.
 *
 * A ragged list per proof: item e of proof p is d_items[p * stride + e * width] (words; width 1 for values, 8 for witness
 * nodes), its count d_count[p * count_stride], at most cap.  fri_witness (width 4) and fri_hash_witness (width 8) hold T
 * lists per proof: tree t of proof p at d_items[p * stride + t * cap * width], its count d_count[p * count_stride + t].
 * The lists point into the buffers as rsv_witness_decommit_dev, rsv_decommit_tree_dev and rsv_fri_open_dev leave them: no
 * staging copy (values of trees 0 .. 2 are three lists into one buffer, each at its tree's offset). */
typedef struct rsv_proof_list {
    const uint32_t* d_items;
    size_t stride;
    const uint32_t* d_count;
    size_t count_stride;
    uint32_t cap;
} rsv_proof_list;
typedef struct rsv_proof_parts {
    uint32_t log_size_plonk, log_size_poseidon, pow_bits, log_blowup, log_last, n_queries, n_layers;
    const uint32_t* d_sums;       /* [n][2][4] */
    const uint32_t* d_roots;      /* [n][3][8] */
    const uint32_t* d_root3;      /* [n][8] */
    const uint32_t* d_samples;    /* [n][134][4] */
    const uint32_t* d_samples3;   /* [n][8][4] */
    const uint32_t* d_nonce;      /* [n][2] */
    const uint32_t* d_fri_roots;  /* [n][T][8] */
    const uint32_t* d_last_poly;  /* [n][2^log_last][4] */
    rsv_proof_list values[4], witness[4];
    rsv_proof_list fri_witness, fri_hash_witness;
} rsv_proof_parts;
/* The length in bytes of a proof with the given counts (HOST, 8 + 2 n_layers of them: values of trees 0 .. 3, witness
 * nodes of trees 0 .. 3, then per layer tree its fri_witness values and its hash_witness nodes).  Host arithmetic: with
 * the capacities it is the bound a caller sizes d_blob with (n times it), with a proof's stored counts the proof's length.
 * NULL counts or bytes: RSV_E_NULL; log_last above RSV_MAX_LOG_LAST_LAYER, n_layers 0 or above 29: RSV_E_SIZE. */
int rsv_proof_bytes(uint32_t log_last, uint32_t n_layers, const uint32_t* counts, size_t* bytes);
/* d_offsets [n + 1] u64: d_offsets[0] = 0, d_offsets[p + 1] - d_offsets[p] the length of proof p — always exact, all
 * multiples of 4: the form rsv_verify_batch_dev requires.  A proof gets a zero-length slot, its neighbours unaffected, when
 * it is masked (d_mask [n] bytes, may be NULL: d_mask[p] == 0) or one of its counts exceeds its cap (nothing is read past
 * a cap).  d_blob NULL: offsets only; the caller may read d_offsets[n] and allocate exactly.  With a d_blob, the bytes of
 * proof p are written iff d_offsets[p + 1] <= blob_cap (bytes): nothing of a proof that does not fit is written, and the
 * caller sees it from d_offsets[n] > blob_cap.  Bytes of d_blob outside the written proofs are left as they were.
 * Three launches: one wave per proof (counts, length, the table of the proof's runs), one workgroup scanning the
 * lengths, one lane per output word (the run found in the proof's table in LDS; dword loads and stores).  The map of the
 * literal words is built on the host for the configuration words and kept in the context: a call under another
 * configuration than the context's last uploads it again.  Refusals before any device work: NULL ctx, parts, d_offsets or
 * any pointer of parts: RSV_E_NULL; n 0 or above 2^20, what rsv_cfg_check refuses of (pow_bits, log_blowup, log_last,
 * n_queries), n_layers 0 or above 29, a pointer (d_blob included) not 4-byte aligned or d_offsets not 8-byte aligned, a
 * stride below cap * width (T * cap * width for the two layer lists, whose count_stride must be at least T), capacities
 * with which one proof exceeds 2^30 words: RSV_E_SIZE.
 * Enqueued on the context's stream with no host synchronisation but the workspace's growth and the map's replacement. */
int rsv_proof_pack_dev(rsv_ctx* ctx, const rsv_proof_parts* parts, size_t n, const uint8_t* d_mask, uint8_t* d_blob, size_t blob_cap,
                       uint64_t* d_offsets);

/* Pack n accept bytes (device) into a little-endian bitmap of ceil(n/32) u32
 * words (device) and return the popcount through *d_count (device u64, may be NULL).
 * This is the buffer the multi-GPU host exchanges with one RCCL all-gather (rsv_exchange_run, below). */
int rsv_accept_bitmap_dev(rsv_ctx* ctx, const uint8_t* d_accept, size_t n,
                          uint32_t* d_bitmap, uint64_t* d_count);

/* ---- e: more than one GPU (BASELINE configs[3]) -----------------------------------------------------------
 * Proofs are independent, so a job shards by contiguous index range and NOTHING is exchanged while it verifies; what is
 * left is to put the shards' accept bits together.  Two layouts, both behind this header:
 *
 * (1) ONE process drives N devices — what the reference's driver is (examples/multi-proofs/src/main.rs:198-295: one
 *     process walks the whole chain).  rsv_multi holds one context per entry of `devices` (a device may be named more
 *     than once: several contexts on one GPU) and runs one host thread per context per call.  A process that owns every
 *     shard has nobody to send to, so the job's accept bytes / bitmap / count are assembled on the host: no collective.
 * (2) One process per GPU (torchrun, MPI, N copies of a Rust binary).  Each rank verifies its shard and the ranks
 *     exchange their bitmap slices with ONE ncclAllGather and their counts with ONE ncclAllReduce over RCCL / xGMI
 *     (rsv_exchange).  RCCL is bound at run time, never linked; RSV_E_UNAVAILABLE where it cannot be loaded.
 *
 * Shard rules (both layouts, and recursive-stwo_amd/sharding.py).  Shards are contiguous index ranges, shard 0 first.
 *   rsv_shard_range   a UNIFORM job (proofs of one shape, or shapes in round-robin order): rank r of `world` owns
 *                     [lo, hi) with sizes differing by at most one, the larger shards first.
 *   rsv_shard_plan    any job, balanced by WORK: bytes are the work (21 - 26.5 proof bytes per permutation over every shape
 *                     of the reference, and the verifier is permutation-bound), so the cut between ranks r - 1 and r is
 *                     the proof boundary nearest to r / world of the job's bytes.  The reference's own job arrives ordered
 *                     by level (examples/multi-proofs/src/main.rs:198-295: 435 KB / 80-query proofs first, 76 KB / 8-query
 *                     ones last): cut by count, rank 0 of 8 gets 4.5 x the bytes of rank 7; cut by bytes, every rank the
 *                     same within one proof.  lens: n proof lengths (HOST); lo, hi: `world` entries each (HOST, written);
 *                     world in 1 .. 4096 (RSV_E_SIZE).  Deterministic: every rank computes the same plan from the same
 *                     lengths.  rsv_multi_verify_batch_host cuts its job this way. */
void rsv_shard_range(size_t n_total, size_t rank, size_t world, size_t* lo, size_t* hi);
int rsv_shard_plan(const uint64_t* lens, size_t n, size_t world, size_t* lo, size_t* hi);

typedef struct rsv_multi rsv_multi;
/* n_devices in 1 .. 64; every entry a valid HIP device index (RSV_E_DEVICE otherwise). */
int rsv_multi_create(const int* devices, size_t n_devices, rsv_multi** out);
void rsv_multi_destroy(rsv_multi* m);
size_t rsv_multi_size(const rsv_multi* m);
/* Context of rank r (owned by m): for rsv_ctx_set_option, or to use a rank on its own.  NULL if out of range. */
rsv_ctx* rsv_multi_ctx(rsv_multi* m, size_t rank);
/* The whole job in HOST memory, as the reference's caller holds it (one serialized buffer per proof): rank r runs
 * rsv_verify_batch_host on shard rsv_shard_range(n, r, size) from its own thread (gather -> pinned -> DMA -> verify,
 * pipelined per device).  accept / reason: n bytes each (reason may be NULL); bitmap: ceil(n / 32) little-endian words
 * (bit i = accept[i]) or NULL; count: accepted proofs or NULL.  cfg->cfg_of (HOST memory here) indexes the whole job.
 * Blocks until every verdict is written.  The first failing rank's status is returned (RSV_E_NOMEM: a rank could not
 * allocate its host staging). */
int rsv_multi_verify_batch_host(rsv_multi* m, const uint8_t* const* proofs, const uint64_t* lens, size_t n,
                                const rsv_cfg_set* cfg, const rsv_public_input* pi, size_t n_pi, uint8_t* accept,
                                uint8_t* reason, uint32_t* bitmap, uint64_t* count);
/* The job already resident in HBM, shard r on the device of context r (the caller chose the split; the job's proof
 * order is shard 0, shard 1, ...).  Pointers are DEVICE pointers of that device, as for rsv_verify_batch_dev;
 * d_cfg_of / d_accept / d_reason may be NULL (no per-proof configuration index / verdict bytes not wanted). */
typedef struct rsv_shard {
    const uint8_t* d_blob;
    const uint64_t* d_offsets;
    size_t n;
    const uint8_t* d_cfg_of;
    uint8_t* d_accept;
    uint8_t* d_reason;
} rsv_shard;
/* n_shards must equal rsv_multi_size(m).  Every context verifies its shard (one pass that also packs the shard's
 * bitmap and count, rsv_hints_out::d_accept_bitmap), the slices come back over PCIe (n / 8 bytes) and are placed at
 * their bit offsets: bitmap = ceil(sum n / 32) HOST words or NULL, count = HOST u64 or NULL.  cfg->cfg_of is ignored
 * (each shard has its own d_cfg_of).  Blocks until all contexts are done. */
int rsv_multi_verify_batch_dev(rsv_multi* m, const rsv_shard* shards, size_t n_shards, const rsv_cfg_set* cfg,
                               const rsv_public_input* pi, size_t n_pi, uint32_t* bitmap, uint64_t* count);

/* Layout (2).  TESTED ON ONE DEVICE ONLY so far (world 1 on hardware, world 2 / 3 / 8 over gloo on CPUs: this pool has
 * one-GPU boxes).  rank 0 obtains an id (ncclGetUniqueId) and hands its RSV_EXCHANGE_ID_BYTES bytes to the other ranks by
 * whatever channel the host has (a file, an environment variable, MPI, a torch store); every rank then calls
 * rsv_exchange_create — collectively: it returns when all `world` ranks have joined (ncclCommInitRank on ctx's device).
 * Per batch: verify the shard with rsv_verify_hints_dev asking for d_accept_bitmap = d_local (a buffer of slice_words
 * words; the verifying pass writes ceil(shard / 32) of them with the bits above the shard zero) and d_accept_count =
 * d_count, then rsv_exchange_run — enqueued on ctx's stream behind the verifying pass, no host synchronisation: it zeroes
 * the words of d_local above the shard's own (a narrower shard than the widest sends slice_words words all the same),
 * afterwards d_gathered [world][slice_words] holds every rank's slice — nothing but accept bits and zeros — and *d_count
 * the job's total on every rank.  rsv_exchange_assemble (pure host arithmetic, no RCCL needed) turns a host copy of
 * d_gathered into the job's accept bytes and / or contiguous bitmap.
 * rsv_exchange_create cuts the job with rsv_shard_range; rsv_exchange_create_plan / rsv_exchange_assemble_plan take the
 * cuts of every rank (lo, hi: `world` entries each, contiguous from 0 — rsv_shard_plan's, or the caller's own;
 * RSV_E_SIZE otherwise), slice_words is then the widest shard's.
 * Lifetime: destroy an exchange BEFORE the context it was created on (it enqueues on that context's stream). */
#define RSV_EXCHANGE_ID_BYTES 128
typedef struct rsv_exchange rsv_exchange;
int rsv_exchange_available(void);     /* 1 if RCCL could be bound in this process, else 0 */
int rsv_exchange_rccl_version(void);  /* ncclGetVersion, 0 if unavailable */
int rsv_exchange_unique_id(uint8_t* id128);
int rsv_exchange_create(rsv_ctx* ctx, const uint8_t* id128, int rank, int world, size_t n_total, rsv_exchange** out);
int rsv_exchange_create_plan(rsv_ctx* ctx, const uint8_t* id128, int rank, int world, const size_t* lo, const size_t* hi,
                             rsv_exchange** out);
void rsv_exchange_destroy(rsv_exchange* x);
/* This rank's [lo, hi) and the slice size every rank contributes (the largest shard's bitmap words, at least 1). */
int rsv_exchange_layout(const rsv_exchange* x, size_t* lo, size_t* hi, size_t* slice_words);
int rsv_exchange_run(rsv_exchange* x, uint32_t* d_local, uint32_t* d_gathered, uint64_t* d_count);
int rsv_exchange_assemble(size_t n_total, size_t world, const uint32_t* gathered, uint8_t* accept, uint32_t* bitmap);
int rsv_exchange_assemble_plan(size_t world, const size_t* lo, const size_t* hi, const uint32_t* gathered, uint8_t* accept,
                               uint32_t* bitmap);

/* Per-stage kernel time of the last rsv_verify_batch_dev on this ctx, measured
 * with HIP events on the ctx stream (ms); all zero unless RSV_OPT_STAGE_TIMES = 1 was set
 * on the context before the call.  names[i] are static strings.
 * Returns the number of stages written (<= cap).  Synchronises the stream. */
int rsv_last_stage_times(rsv_ctx* ctx, const char** names, float* ms, int cap);

#ifdef __cplusplus
}
#endif
#endif /* RSV_H_ */
