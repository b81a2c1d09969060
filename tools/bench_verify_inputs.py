#!/usr/bin/env python3
"""rsv_verify_batch_dev (one table of public inputs for the batch) beside rsv_verify_batch_inputs_dev (every proof its own,
here the same records replicated) in one session, and the statement-sum kernel alone (rsv_public_input_sum_dev).  The batch
is bench.py's (its fixtures round-robin, its seeded tampering, built in HBM); n_pi = 3 is the standard inputs, a larger n_pi
appends random records (every proof is then rejected at the logup balance by both calls alike, with the same work done).
Times are HIP events on the context's stream around each call, interleaved (tools/chain_bench.py).  One JSON line per
(proofs, n_pi).

--shared-only times the shared call alone and uses nothing this change added, so that the same file runs in a checkout
of the commit before it, against that commit's library.

    python tools/bench_verify_inputs.py [--cases 1:3,1024:3,65536:3,1:1024,1024:1024] [--steps 10] [--warmup 2] [--shared-only]"""
import argparse
import json

import numpy as np

import chain_bench as CB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1:3,1024:3,65536:3,1:1024,1024:1024", help="proofs:n_pi, comma separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shared-only", action="store_true")
    args = ap.parse_args()
    import torch
    import rsvload
    rsv = rsvload.load_package()
    import bench
    if rsv.device_count() < 1:
        raise SystemExit("bench_verify_inputs needs a HIP device")
    dev = torch.device("cuda", 0)
    ctx = rsv.Context(0)
    cfgs = bench.fixture_configs(rsv, bench.FIXTURES)
    rnd = np.random.default_rng(1)
    for case in args.cases.split(","):
        n, n_pi = (int(x) for x in case.split(":"))
        d_blob, d_offsets, _, _, idx = bench.build_batch_on_device(torch, dev, n, 0)
        cfg = ctx.prepare_cfg([cfgs[int(k)] for k in idx], n)
        shared = list(rsv.STANDARD_INPUTS)[:n_pi]
        shared += [(int(rnd.integers(4, 1 << 20)), tuple(int(x) for x in rnd.integers(0, 0x7FFFFFFF, 4))) for _ in range(n_pi - len(shared))]
        rec = np.array([[k] + list(v) for k, v in shared], dtype=np.uint32).reshape(1, n_pi, 5)
        d_inputs = torch.from_numpy(rec.view(np.int32)).to(dev).repeat(n, 1, 1).contiguous()
        d_za = torch.from_numpy(rnd.integers(0, 0x7FFFFFFF, (n, 8)).astype(np.int32)).to(dev)
        d_sum = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        out = {k: (torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)) for k in ("shared", "per_proof")}
        calls = {
            "shared": lambda: ctx.verify_batch(d_blob, d_offsets, n, *out["shared"], cfg=cfg, inputs=shared),
            "per_proof": lambda: ctx.verify_batch(d_blob, d_offsets, n, *out["per_proof"], cfg=cfg, d_inputs=d_inputs, n_inputs=n_pi),
            "sum_alone": lambda: ctx.public_input_sum(d_inputs, n, n_pi, d_za, d_sum),
        }
        if args.shared_only:
            calls = {"shared": calls["shared"]}
        times, med = CB.time_interleaved(ctx, calls, args.steps, args.warmup)
        ctx.synchronize()
        same = args.shared_only or all(torch.equal(a, b) for a, b in zip(out["shared"], out["per_proof"]))
        print(json.dumps({"proofs": n, "n_pi": n_pi, "steps": args.steps, "verdicts_equal": bool(same),
                          "accepted": int(out["shared"][0].sum().item()),
                          "ms_median": {k: round(v, 4) for k, v in med.items()},
                          "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
                          "ms_max": {k: round(float(np.max(v)), 4) for k, v in times.items()},
                          "per_proof_over_shared": None if args.shared_only else round(med["per_proof"] / med["shared"], 4),
                          "input_bytes": n * n_pi * 20}), flush=True)
        assert same, "the per-proof call's verdicts differ from the shared call's"
        del d_blob, d_offsets, d_inputs, d_za, d_sum, out
    ctx.close()


if __name__ == "__main__":
    main()
