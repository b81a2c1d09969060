#!/usr/bin/env python3
"""Throughput of rsv_witness_commit_dev (trees 0, 1 and 2 of the next proof: interpolation, LDE, Merkle roots, the
interaction columns and the transcript draws between them), one JSON line.

    python tools/bench_commit.py --fixture level9-1.bin --log-blowup 8 --proofs 1 --steps 5

The next proof's shape is what the fixture's program gives (level9-1.bin -> the level10 shape, lp/lq 16/15; level11-1.bin
-> level12; small_proof.bin -> recursive_16_15) and `--log-blowup` is the next configuration's.  The trace columns are put
in HBM once (rsv_witness_eval_dev + rsv_witness_trace_dev); timed is the commit call alone.

Permutations per proof are COUNTED FROM SHAPES (`perms_per_proof` below): a leaf of c columns costs ceil(c/8) + 1
permutations, a node with c columns 1 + ceil(c/8) + 1, a plain node 1; the rate is compared with the 9.5 G permutations/s
that k_permute sustains.  HBM bytes are ALGORITHMIC: per tree the LDE written once by the FFT and read once by the leaf
and node hashes, each global butterfly pass above the 4 096-point LDS stage reading and writing it once more, and the node
layers written and read once (32 B each); against 8 TB/s.  `bound` is whichever fraction is the larger.  For a per-kernel
split run the tool under `rocprofv3 --kernel-trace --stats -- python tools/bench_commit.py ...`."""
import argparse
import json

from chain_bench import add_args, open_chain, time_interleaved

PEAK_GBS = 8000.0
PERM_RATE = 9.5e9
LDS_LOG = 12
TREES = ((10, 40), (12, 48), (8, 8))  # (Plonk, Poseidon) columns of trees 0, 1, 2


def tree_work(layers, b):
    """layers: {log size (before blowup): n_cols} -> (permutations, algorithmic HBM bytes) of one commitment."""
    cols_at = {log + b: c for log, c in layers.items()}
    top = max(cols_at)
    perms = 0
    for l in range(top + 1):
        c = cols_at.get(l, 0)
        sponge = -(-c // 8)
        perms += (1 << l) * ((sponge + 1) if l == top else (1 + (sponge + 1 if c else 0)))
    lde_words = sum(c << (log + b) for log, c in layers.items())
    passes = sum((c << (log + b)) * (1 + max(0, log - LDS_LOG)) for log, c in layers.items())
    nodes = sum(1 << l for l in range(top + 1))
    byts = 4 * (sum(c << log for log, c in layers.items()) + lde_words + 2 * passes) + 64 * nodes
    return perms, byts


def perms_per_proof(lp, lq, b):
    tot_p = tot_b = 0
    for cp, cq in TREES:
        layers = {lp: cp, lq: cq} if lp != lq else {lp: cp + cq}
        p, by = tree_work(layers, b)
        tot_p, tot_b = tot_p + p, tot_b + by
    return tot_p + 8, tot_b  # + the transcript's 8 permutations


def main():
    ap = argparse.ArgumentParser()
    add_args(ap, "level9-1.bin", 8)
    args = ap.parse_args()
    rsv, ctx, wp, ch = open_chain(args, "trace")
    lp, lq, n, b = ch.lp, ch.lq, ch.n, ch.log_blowup
    # the chain allocates commit()'s tensors in its first call: with --warmup 0 that is the first timed one
    times, med = time_interleaved(ctx, {"commit": ch.commit}, args.steps, args.warmup)
    times, ms = times["commit"], med["commit"]
    ok = int(ch.ok.sum().item())
    perms, byts = perms_per_proof(lp, lq, b)
    perm_frac = perms * n / (ms * 1e-3) / PERM_RATE
    hbm_frac = byts * n / (ms * 1e-3) / (PEAK_GBS * 1e9)
    print(json.dumps({"tool": "bench_commit", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "log_blowup": b, "proofs": n,
                      "ok": ok, "ms_per_call": round(ms, 3), "ms_all": [round(t, 3) for t in times], "perms_per_proof": perms,
                      "perm_rate_g": round(perms * n / (ms * 1e-3) / 1e9, 3), "perm_rate_fraction": round(perm_frac, 3),
                      "hbm_bytes_per_proof": byts, "hbm_fraction": round(hbm_frac, 3),
                      "bound": "permutations" if perm_frac >= hbm_frac else "HBM"}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
