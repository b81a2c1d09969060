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
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    ap.add_argument("--fixture", default="level9-1.bin")
    ap.add_argument("--log-blowup", type=int, default=8)
    ap.add_argument("--proofs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--copies", type=int, default=1)
    args = ap.parse_args()
    import rsvload
    rsv = rsvload.load_package()
    import torch
    import bench
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        man = {e["file"]: e for e in json.load(f)["proofs"]}
    e = man[args.fixture]
    inputs = [(i, tuple(v)) for i, v in e["inputs"]]
    cfg = rsv.PcsConfig(e["pow_bits"], e["log_blowup_factor"], e["log_last_layer_degree_bound"], e["n_queries"])
    proof = bench.read_fixture(args.fixture)
    wp = rsv.WitnessProgram.build(proof, cfg, inputs, copies=args.copies)
    lp, lq = wp.trace_sizes()
    F = wp.shape.flow_count
    n_ops = len(wp.gates()[1])
    n, b = args.proofs, args.log_blowup
    dev = torch.device("cuda:0")
    blob, offsets = rsv.pack([proof] * n)
    ctx = rsv.Context(0)
    d_blob, d_off = torch.from_numpy(blob.copy()).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_vars = torch.zeros((n, wp.n_vars, 4), dtype=torch.int32, device=dev)
    d_flow = torch.zeros((n, F, 32), dtype=torch.int32, device=dev)
    d_swap = torch.zeros((n, F), dtype=torch.uint8, device=dev)
    d_acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    ctx.witness(wp, d_blob, d_off, n, d_vars, d_acc, inputs=inputs, d_flow=d_flow, d_flow_swap=d_swap)
    d_plonk = torch.zeros((n, 12, 1 << lp), dtype=torch.int32, device=dev)
    d_pos = torch.zeros((n, 48, 1 << lq), dtype=torch.int32, device=dev)
    d_ops = torch.zeros((n, max(n_ops, 1)), dtype=torch.int32, device=dev)
    ctx.witness_trace(wp, d_vars, d_acc, n, d_plonk=d_plonk, d_poseidon=d_pos, d_ops=d_ops, d_flow=d_flow, d_flow_swap=d_swap)
    del d_vars, d_flow, d_swap, d_blob
    d_roots = torch.zeros((n, 3, 8), dtype=torch.int32, device=dev)
    d_draws = torch.zeros((n, 12), dtype=torch.int32, device=dev)
    d_ip = torch.zeros((n, 8, 1 << lp), dtype=torch.int32, device=dev)
    d_iq = torch.zeros((n, 8, 1 << lq), dtype=torch.int32, device=dev)
    d_sums = torch.zeros((n, 2, 4), dtype=torch.int32, device=dev)
    d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    call = lambda: ctx.witness_commit(wp, d_plonk, d_pos, d_ops, d_acc, n, b, d_roots, d_draws, d_ip, d_iq, d_sums, d_ok=d_ok)  # noqa: E731
    for _ in range(args.warmup):
        call()
    ctx.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.current_stream()
    times = []
    for _ in range(args.steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        call()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    ok = int(d_ok.sum().item())
    ms = float(np.median(times))
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
