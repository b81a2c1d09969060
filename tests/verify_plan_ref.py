"""The form decisions of a verify call as the launcher took them INLINE, before they became one host-side plan
(recursive-stwo_amd/csrc/host_logic.hpp: plan_batch, plan_launches, plan_group): a restatement in Python of the text of
verify_impl at commit 4da6cb5, the last one that had them between its launches.  The numbers in the comments are line
numbers of recursive-stwo_amd/csrc/verify_api.inc at that commit (`git show 4da6cb5:recursive-stwo_amd/csrc/verify_api.inc`),
so that each statement here can be held against the statement it restates.  Written from that text, not from the plan
functions: tests/test_host_logic_asan.py compares the two over every batch size at which a form changes.

A case is what the decisions depend on: the options, the batch size, the configuration set as values, the outputs asked
for, and (for the second step) the groups' entries.  plan_line() returns the line tests/host_logic_asan.cpp prints for it."""

MAXQ = 128                          # layout.hpp
MAX_FUSED = 16                      # k_plan.hpp
K_BLOCK = 256                       # :22
K_ROW_TREE_BLOCK = 512              # :25
K_ROW_TREE_LANES = 256 * 16 * 9     # :26
K_ROW_QUERY_LANES = 256 * 16        # :27

# Options (rsv_hip.hip at that commit, :49-76): the ones verify_impl read for a form, each with the values
# rsv_ctx_set_option accepts besides its default (for RSV_OPT_WS_BUDGET_MB, 1 .. 2^20: both ends and one between)
DEFAULTS = {"transcript_form": 0, "transcript_split": 0, "oods_form": 0, "qconst_form": 0, "plan_form": 0, "tree_cap": 0,
            "overlap_trees": 0, "critical_chain": 0, "device_order": 0, "flow_cap": 0, "query_form": 0, "tree_pace": 0,
            "pair_order": 0, "cap_mid": 0, "cap_top": 0, "ws_budget_mb": 8192}
ACCEPTED = {name: (1, 2) for name in DEFAULTS}
ACCEPTED["tree_pace"] = (1, 2, 3)
ACCEPTED["ws_budget_mb"] = (1, 512, 1 << 20)


def grid_for(n, block):             # rsv_hip.hip: grid_for
    return (n + block - 1) // block


def step_one(o, N, n_cfgs, cfg_of, log_blowup, log_last, n_queries, flow, paths, trace_sib, pair_sib):
    """What verify_impl decided before the groups were known.  (`own` chose nothing but the OODS kernel's input type.)"""
    row = N <= 24576                                                                            # :267
    if o["transcript_form"]:                                                                    # :268
        row = o["transcript_form"] == 1
    split = row and not flow and (o["transcript_split"] == 2 if o["transcript_split"] else N <= 4096)   # :279
    # :302-313: k_transcript<false, true>, the paced lane form, is the ladder's last rung
    paced = not split and not (row and flow) and not row and not flow and not N <= 49152
    device_order = (n_cfgs == 1 and not cfg_of and not paths and o["device_order"] != 2 and n_queries >= 1 and   # :325
                    n_queries <= MAXQ and log_blowup >= 1 and log_blowup <= 16 and log_last <= 16)               # :326
    tree_form = 1                                                                               # :345
    nq_est = 4 if n_queries < 4 else n_queries                                                  # :347
    fold_est = log_blowup + log_last
    lanes = N * nq_est * (22 - fold_est if 22 > fold_est else 1)                                # :348
    if o["tree_pace"]:                                                                          # :349
        tree_form = 1 if o["tree_pace"] == 1 else (0 if o["tree_pace"] == 2 else 2)
    elif n_cfgs == 1 and lanes <= K_ROW_TREE_LANES:                                             # :350
        tree_form = 2
    elif n_cfgs == 1 and lanes <= 1024 * 16 * 9:                                                # :351
        tree_form = 0
    if flow and tree_form == 0:                                                                 # :352
        tree_form = 1
    small_trees = tree_form != 1                                                                # :354
    qconst4 = N <= 4096 and o["qconst_form"] != 1                                               # :424
    qrow = o["qconst_form"] == 1 if o["qconst_form"] else N <= 24576                            # :428
    oods_row = o["oods_form"] == 1 if o["oods_form"] else N <= 6144                             # :167, :446
    cap_top = not (trace_sib or pair_sib) and (o["cap_top"] == 1 if o["cap_top"] else N >= 1024)   # :464
    # :466, and ws_budget() at :101
    policy = (o["ws_budget_mb"] << 20, MAX_FUSED, o["tree_cap"] == 2, flow, o["flow_cap"] == 2, cap_top, o["cap_mid"])
    serial_plan = o["plan_form"] == 2                                                           # :474
    pair_deal = o["pair_order"] != 2                                                            # :594
    return (row, split, paced, device_order, tree_form, small_trees, qrow, qconst4, oods_row, cap_top, serial_plan, pair_deal) + policy


def step_two(o, one, N, n_cfgs, log_blowup, log_last, n_queries, flow, pair_sib, groups):
    """What verify_impl decided once plan_groups had cut the batch.  groups: lists of entries (G, cn, maxM, maxInner), the
    last two the entry's bucket's."""
    device_order, tree_form, qrow, serial_plan = one[3], one[4], one[6], one[10]
    for grp in groups:                                                                          # :475
        for (G, _, _, _) in grp:                                                                # :476
            if tree_form == 2 and G > K_ROW_TREE_BLOCK // 16:                                   # :477
                tree_form = 1 if flow else 0
    tree_lanes = K_ROW_TREE_BLOCK // 16 if tree_form == 2 else K_BLOCK                          # :478
    overlap_trees = len(groups) == 1                                                            # :485
    if o["overlap_trees"] == 2:                                                                 # :486
        overlap_trees = False
    chain = overlap_trees and (o["critical_chain"] == 1 if o["critical_chain"] else N <= 24576)   # :493
    query_row = chain and (o["query_form"] == 1 if o["query_form"] else                         # :496
                           N * (4 if n_queries < 4 else n_queries) <= K_ROW_QUERY_LANES and n_cfgs == 1)
    for grp in groups:                                                                          # :497
        for (G, _, _, _) in grp:                                                                # :498
            if G > K_ROW_TREE_BLOCK // 16:                                                      # :499
                query_row = False
    qconst_in_plan = chain and not serial_plan and (o["qconst_form"] == 1 if o["qconst_form"] else N <= 24576)   # :500
    # :693 (inside the loop over the groups, which a batch with overlap_trees runs once; not reached in the chain layout: :675)
    # launches the OODS kernel on the main stream; what is left for :706 goes to the side stream
    oods_on_main = overlap_trees and not chain
    out = [(tree_form, tree_lanes, overlap_trees, chain, query_row, qconst_in_plan, oods_on_main)]
    for grp in groups:
        top_t = top_p = max_inner = 0                                                           # :512
        for (_, cn, _, maxInner) in grp:
            top_t += grid_for(cn * 4, 256)                                                      # :560
            top_p += grid_for(cn * (1 + maxInner), 256)                                         # :561
            max_inner = max(max_inner, maxInner)                                                # :576
        group_M, live = 0, 1 + max_inner                                                        # :583
        for (_, _, maxM, _) in grp:                                                             # :584
            group_M = max(group_M, maxM)
        if device_order:                                                                        # :585
            group_M = 22                                                                        # :589
            fold = log_blowup + log_last                                                        # :590
            live = group_M - fold if group_M > fold else 1                                      # :591
        tm_t, tm_p = top_t * 256 >= 1 << 19, top_p * 256 >= 1 << 19                             # :602
        pair_lds = K_BLOCK * 32 if (pair_sib or flow) else 0                                    # :621
        out.append((tm_t, tm_p, pair_lds, group_M, live))
    return out


ONE_FMT = " %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d :"
TWO_FMT = " %d %d %d %d %d %d %d"
GROUP_FMT = " : %d %d %d %d %d"


def plan_line(key, one, two):
    """The line of tests/host_logic_asan.cpp (mode `plan`) for one case.  key: the text that names the case; one: ONE_FMT % the
    first step's fields (the same for every set of groups)."""
    return key + one + TWO_FMT % two[0] + "".join([GROUP_FMT % g for g in two[1:]])
