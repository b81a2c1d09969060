#!/usr/bin/env python3
"""Time of the commit phase of FRI of the next proof beside the commitment of trees 0-2 of the same proof in the same run,
one JSON line.

    python tools/bench_fri.py --fixture level10-1.bin --log-blowup 1 --log-last 0 --proofs 16 --steps 5

Timed interleaved, `--steps` rounds, HIP events on the context's stream, medians:
  commit       rsv_witness_commit_dev on the chain's buffers (the yardstick: its forward FFT of the 126 columns is what
               the quotient call does again);
  fri          rsv_witness_fri_dev on what tree 3 and the sampling left (the channel is restored before every call):
               the sample mixes, the quotient columns and the layers;
  fri_commit   rsv_fri_commit_dev alone on the quotient columns that call left.
`quotients` is fri - fri_commit.  The shares of the row kernel (k_fr_rows), the extension (k_cm_fft_*), the layer trees
(k_fr_hash_layer), the folds (k_fr_fold) and the channel steps (k_fr_draw) are the rows of
`rocprofv3 --kernel-trace --stats -- python tools/bench_fri.py ...`."""
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
    ap.add_argument("--log-last", type=int, default=0)
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
    ctx.witness_tree3(wp, d_plonk, d_pos, d_ops, d_ip, d_iq, d_acc, n, b, d_sums, d_draws, d_chan0, d_comp, d_root3, d_oods, d_samples3, d_ok=d_ok)
    d_samples = z(n, 134, 4)
    ctx.witness_sample(wp, d_plonk, d_pos, d_ops, d_ip, d_iq, d_acc, n, d_oods, d_samples, d_ok=d_ok)
    sz = rsv.fri_sizes(lp, lq, b, args.log_last)
    ni = sz["n_inner"]
    d_after, d_quot, d_froots, d_alphas = z(n, 4), z(n, sz["quot_words"]), z(n, 1 + ni, 8), z(n, 1 + ni, 4)
    d_layers, d_last = z(n, max(sz["layer_words"], 1)), z(n, 1 << args.log_last, 4)
    d_low = torch.zeros(n, dtype=torch.uint8, device=dev)

    def fri():
        d_chan.copy_(d_chan0)
        ctx.witness_fri(wp, d_plonk, d_pos, d_ops, d_ip, d_iq, d_acc, n, b, args.log_last, d_comp, d_oods, d_samples, d_samples3, d_chan,
                        d_after, d_quot, d_froots, d_alphas, d_layers, d_last, d_low, d_ok=d_ok)

    calls = {
        "commit": lambda: ctx.witness_commit(wp, d_plonk, d_pos, d_ops, d_acc, n, b, d_roots, d_draws, d_ip, d_iq, d_sums, d_ok=d_ok),
        "fri": fri,
        "fri_commit": lambda: ctx.fri_commit(d_quot, sz["sizes"], b, args.log_last, n, d_chan, d_froots, d_alphas, d_layers, d_last, d_low,
                                             d_mask=d_ok),
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
    positions = sum(1 << s for s in sz["sizes"])
    print(json.dumps({"tool": "bench_fri", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "sizes": sz["sizes"], "n_inner": ni,
                      "log_blowup": b, "log_last": args.log_last, "proofs": n, "ok": ok, "low_degree": int(d_low.sum().item()),
                      "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
                      "quotients_ms": round(med["fri"] - med["fri_commit"], 4), "fri_over_commit": round(med["fri"] / med["commit"], 5),
                      "quotient_positions_per_proof": positions}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
