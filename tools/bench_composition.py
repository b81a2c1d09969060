#!/usr/bin/env python3
"""Time of rsv_witness_tree3_dev (tree 3 of the next proof: the composition columns, their commitment, the OODS point and
the eight sampled values) and of rsv_composition_dev alone, beside the commitment of trees 0-2 of the same shapes in the
same run, one JSON line.

    python tools/bench_composition.py --fixture level10-1.bin --log-blowup 1 --proofs 16 --steps 5

Timed interleaved, `--steps` rounds, HIP events on the context's stream, medians:
  commit       rsv_witness_commit_dev on the chain's buffers (the yardstick: it interpolates the same 126 columns and
               extends them by 2^log_blowup, where the composition extends them to 2^clb rows);
  tree3        rsv_witness_tree3_dev on what the commitment left (the channel is restored before every call);
  composition  rsv_composition_dev on the same columns, the program's preprocessed columns shared by every proof (the op
               column's witness rows are the template's: the work is the same).
The shares of the row kernels (k_co_plonk, k_co_poseidon), the extension (k_cm_fft_*) and the tree (k_cm_hash_layer, k_cm_top)
are the rows of `rocprofv3 --kernel-trace --stats -- python tools/bench_composition.py ...`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="level10-1.bin")
    ap.add_argument("--log-blowup", type=int, default=1)
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
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    d_roots, d_draws, d_ip, d_iq, d_sums = z(n, 3, 8), z(n, 12), z(n, 8, 1 << lp), z(n, 8, 1 << lq), z(n, 2, 4)
    d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_chan0, d_chan = z(n, 16), z(n, 16)
    ctx.witness_commit(wp, d_plonk, d_pos, d_ops, d_acc, n, b, d_roots, d_draws, d_ip, d_iq, d_sums, d_channel=d_chan0, d_ok=d_ok)
    L3 = rsv.composition_log_size(lp, lq)
    d_comp, d_root3, d_oods, d_samples3 = z(n, 8, 1 << L3), z(n, 8), z(n, 8), z(n, 8, 4)
    ppre, qpre = wp.preprocessed()
    d_ppre = torch.from_numpy(np.ascontiguousarray(ppre, dtype=np.uint32).view(np.int32)).to(dev)
    d_qpre = torch.from_numpy(np.ascontiguousarray(qpre, dtype=np.uint32).view(np.int32)).to(dev)

    def tree3():
        d_chan.copy_(d_chan0)
        ctx.witness_tree3(wp, d_plonk, d_pos, d_ops, d_ip, d_iq, d_acc, n, b, d_sums, d_draws, d_chan, d_comp, d_root3, d_oods, d_samples3,
                          d_ok=d_ok)

    calls = {
        "commit": lambda: ctx.witness_commit(wp, d_plonk, d_pos, d_ops, d_acc, n, b, d_roots, d_draws, d_ip, d_iq, d_sums, d_ok=d_ok),
        "tree3": tree3,
        "composition": lambda: ctx.composition(lp, lq, (d_ppre, d_plonk, d_ip), (d_qpre, d_pos, d_iq), d_sums, d_draws, n, d_comp, d_mask=d_ok),
    }
    for _ in range(max(args.warmup, 1)):
        for call in calls.values():
            call()
    ctx.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.current_stream()
    times = {k: [] for k in calls}
    for _ in range(args.steps):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    ok = int(d_ok.sum().item())
    print(json.dumps({"tool": "bench_composition", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "log_composition": L3,
                      "log_blowup": b, "proofs": n, "ok": ok, "ms": {k: round(v, 4) for k, v in med.items()},
                      "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
                      "tree3_over_commit": round(med["tree3"] / med["commit"], 5),
                      "composition_over_tree3": round(med["composition"] / med["tree3"], 5)}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
