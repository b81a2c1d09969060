// options.hpp — the option table of a context (include/rsv.h: rsv_option).  Plain C++ (ints and long longs only): read by
// the library (rsv_hip.hip) and by the launch plan of a verify call (host_logic.hpp), which a sanitizer build compiles
// without HIP.
#pragma once

// Options (include/rsv.h: rsv_option).  Nothing in this library reads the environment: a knob is set through
// rsv_ctx_set_option, on one context or (ctx == NULL) as the process default that contexts created later inherit.
struct Options {
    int transcript_form = 0;   // 0 auto (by batch size), 1 row, 2 lane
    int transcript_split = 0;  // row form: 0 auto, 1 one launch, 2 front + back
    int oods_form = 0, qconst_form = 0;  // 0 auto, 1 row, 2 lane
    int plan_form = 0;         // 0 / 1 one lane per (proof, query), 2 one lane per proof (the original)
    int tree_cap = 0;          // 0 / 1 dense top-of-tree cap, 2 every path walks to the root
    int overlap_trees = 0;     // 0 / 1 FRI trees beside the trace trees, 2 behind them
    long long ws_budget_mb = 8192;
    int perm_wg_per_cu = 24;
    long long host_chunk_mb = 256;
    int host_threads = 0;      // 0 = min(cores, 4)
    int critical_chain = 0;    // 0 auto, 1 the chain of dependent kernels on ONE stream, 2 the round-2 stream layout
    int device_order = 0;      // 0 / 1 single-configuration batches: slot order on the device, no host round trip; 2 host
    int witness_layout = 0;    // 0 / 1 d_variables [proof][variable], 2 [variable][proof]
    int flow_cap = 0;          // PoseidonFlow passes: 0 / 1 top-of-tree cap (shared nodes hashed once), 2 every lane walks to the root
    int query_form = 0;        // 0 auto (by batch size), 1 k_query with a row of 16 threads per query, 2 with one lane per query
    int stage_times = 0;       // 0 / 2 off, 1 record an event pair around every stage (rsv_last_stage_times)
    int tree_pace = 0;         // 0 auto (by batch size), 1 the tree kernels on the paced permutation instances, 2 on the unpaced ones, 3 in the row form (16 threads per path)
    int pair_order = 0;        // 0 / 1 the FRI trees of a small launch dealt out over the compute units, 2 grid row y = tree y
    int cap_mid = 0;           // 0 auto (buckets whose in-kernel cap levels fill their waves badly), 1 every bucket hands over at the cap level (k_cap_mid + k_cap_top), 2 none
    int cap_top = 0;           // 0 auto (batches of >= 1 024 proofs), 1 the last levels of every tree in k_cap_top, 2 inside the Merkle kernels
    long long witness_small_max = 0;  // 0 default, else 1 + the largest batch that runs the program in one launch
    int witness_small_log = 0;        // 0 default, else 1 + log2(proofs per workgroup) of that form
    int witness_walk_log = 0;         // level form: 0 auto, 1 off, else 1 + log2(proofs per workgroup) of the one-launch tail
    int circuit_eval_form = 0;        // rsv_circuit_eval_dev: 0 auto (by batch size), 1 a launch per level, 2 a workgroup per witness walks the levels
    long long statement_row_max = 0;  // rsv_statement_digest_dev: 0 default, else 1 + the largest number of groups hashed in the row form
    int ws_fill = 0;                  // diagnostic: 0 off, else 1 + the byte every workspace is filled with before a call carves it (ensure_buf)
};
