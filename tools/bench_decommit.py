#!/usr/bin/env python3
"""Time of rsv_witness_decommit_dev (the openings of trees 0, 1 and 2 of the next proof at n_queries positions) beside the
commitment of the same trees at the same commit, one JSON line.

    python tools/bench_decommit.py --fixture level9-1.bin --log-blowup 8 --queries 16 --proofs 1 --steps 5

There is no earlier opening to compare with, so the yardstick is rsv_witness_commit_caps_dev on the same buffers: the three
calls (commitment, opening without caps, opening with caps) are timed interleaved, `--steps` rounds.  Without caps the
opening recomputes every block, about one commitment without the interaction columns; with caps only the blocks the queries
touch, `touched_blocks` of 2^log_blowup per tree (counted on the host from the positions, per proof: the queries are random
and differ per proof), plus the plan and gather launches.  For a per-kernel split run the tool under
`rocprofv3 --kernel-trace --stats -- python tools/bench_decommit.py ...`."""
import argparse
import json

import numpy as np
from chain_bench import add_args, open_chain, time_interleaved


def main():
    ap = argparse.ArgumentParser()
    add_args(ap, "level9-1.bin", 8)
    ap.add_argument("--queries", type=int, default=16)
    args = ap.parse_args()
    rsv, ctx, wp, ch = open_chain(args, "trace", caps=True)
    import torch
    lp, lq, n, b, nq = ch.lp, ch.lq, ch.n, ch.log_blowup, args.queries
    top = max(lp, lq) + b
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=ch.device)  # noqa: E731
    vcaps, wcap = rsv.witness_decommit_sizes(wp, b, nq)
    q = np.random.default_rng(1).integers(0, 1 << top, (n, nq)).astype(np.uint32)
    d_q = torch.from_numpy(q.view(np.int32)).to(ch.device)
    d_v, d_nv, d_w, d_nw = z(n, sum(vcaps)), z(n, 3), z(n, 3, wcap, 8), z(n, 3)
    touched = [len(set((row >> (top - b)).tolist())) for row in q]
    calls = {
        "commit": ch.commit,
        "open_no_caps": lambda: ch.decommit(d_q, d_v, d_nv, d_w, d_nw, caps=False),
        "open_caps": lambda: ch.decommit(d_q, d_v, d_nv, d_w, d_nw),
    }
    times, med = time_interleaved(ctx, calls, args.steps, max(args.warmup, 1))
    share = float(np.mean(touched)) / (1 << b)
    print(json.dumps({"tool": "bench_decommit", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "log_blowup": b, "proofs": n,
                      "queries": nq, "ok": int(ch.ok.sum().item()), "touched_blocks_mean": round(float(np.mean(touched)), 2),
                      "block_share": round(share, 4), "n_values": d_nv[0].cpu().tolist(), "n_witness": d_nw[0].cpu().tolist(),
                      "ms": {k: round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(t, 3) for t in v] for k, v in times.items()},
                      "open_caps_over_commit": round(med["open_caps"] / med["commit"], 4),
                      "open_no_caps_over_commit": round(med["open_no_caps"] / med["commit"], 4)}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
