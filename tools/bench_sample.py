#!/usr/bin/env python3
"""Time of rsv_witness_sample_dev (sampled_values[0..2] of the next proof at the OODS point) and of rsv_sample_tree_dev
from coefficients, beside the commitment of the same trees at the same commit, one JSON line.

    python tools/bench_sample.py --fixture level9-1.bin --log-blowup 8 --proofs 1 --steps 5

Timed interleaved, `--steps` rounds, HIP events on the context's stream, medians:
  commit         rsv_witness_commit_dev on the chain's buffers (the yardstick; it interpolates the same 126 columns);
  sample         rsv_witness_sample_dev: interpolation in the workspace (RSV_SAMPLE_COLUMNS) + the dot products;
  coeffs_t1, t2  rsv_sample_tree_dev with RSV_SAMPLE_COEFFS on the per-proof buffers of trees 1 (60 columns, one point) and
                 2 (16 columns, two points), read as coefficients (any canonical words are; the traffic is what a
                 commitment's d_coeffs would give): 4 bytes per coefficient, `coeffs_share_of_8TBs` = that over the time
                 over the 8 TB/s peak;
  coeffs_t0      the same on tree 0's 50 columns, 49 of them one set shared by every proof (mostly cache traffic).
The interpolation alone is the k_cm_fft_* rows of `rocprofv3 --kernel-trace --stats -- python tools/bench_sample.py ...`."""
import argparse
import json

import numpy as np
from chain_bench import add_args, open_chain, time_interleaved


def main():
    ap = argparse.ArgumentParser()
    add_args(ap, "level9-1.bin", 8)
    args = ap.parse_args()
    rsv, ctx, wp, ch = open_chain(args, "trace")
    import torch
    lp, lq, n, b = ch.lp, ch.lq, ch.n, ch.log_blowup
    dev = ch.device
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    rng = np.random.default_rng(1)
    d_oods = torch.from_numpy(rng.integers(0, 0x7FFFFFFF, (n, 8)).astype(np.int32)).to(dev)
    d_pts2 = torch.from_numpy(rng.integers(0, 0x7FFFFFFF, (n, 2, 8)).astype(np.int32)).to(dev)
    ppre, qpre = wp.preprocessed()
    d_ppre = torch.from_numpy(np.ascontiguousarray(ppre, dtype=np.uint32).view(np.int32)).to(dev)
    d_qpre = torch.from_numpy(np.ascontiguousarray(qpre, dtype=np.uint32).view(np.int32)).to(dev)
    t0 = [{"log_size": lp, "d_cols": d_ppre, "n_cols": 10, "proof_stride": 0}, {"log_size": lq, "d_cols": d_qpre, "n_cols": 40, "proof_stride": 0}]
    t1 = [{"log_size": lp, "d_cols": ch.plonk, "n_cols": 12}, {"log_size": lq, "d_cols": ch.poseidon, "n_cols": 48}]
    # the interaction columns are there once the first commit of the rounds below has run
    t2 = lambda: [{"log_size": lp, "d_cols": ch.int_plonk, "n_cols": 8}, {"log_size": lq, "d_cols": ch.int_poseidon, "n_cols": 8}]  # noqa: E731
    o0, o1, o2 = z(n, 1, 50, 4), z(n, 1, 60, 4), z(n, 2, 16, 4)
    calls = {
        "commit": ch.commit,
        "sample": lambda: ch.sample(d_oods),
        "coeffs_t0": lambda: ctx.sample_tree(t0, n, d_oods, 1, o0, d_mask=ch.ok, source=rsv.SAMPLE_COEFFS),
        "coeffs_t1": lambda: ctx.sample_tree(t1, n, d_oods, 1, o1, d_mask=ch.ok, source=rsv.SAMPLE_COEFFS),
        "coeffs_t2": lambda: ctx.sample_tree(t2(), n, d_pts2, 2, o2, d_mask=ch.ok, source=rsv.SAMPLE_COEFFS),
    }
    times, med = time_interleaved(ctx, calls, args.steps, max(args.warmup, 1))
    ok = int(ch.ok.sum().item())
    coeff_bytes = 4 * ok * ((12 + 8) * (1 << lp) + (48 + 8) * (1 << lq))  # trees 1 and 2, every word once
    coeff_ms = med["coeffs_t1"] + med["coeffs_t2"]
    print(json.dumps({"tool": "bench_sample", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "log_blowup": b, "proofs": n, "ok": ok,
                      "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
                      "coeffs_t1_t2_bytes": coeff_bytes, "coeffs_t1_t2_ms": round(coeff_ms, 4),
                      "coeffs_share_of_8TBs": round(coeff_bytes / (coeff_ms * 1e-3) / 8e12, 4) if coeff_ms > 0 else None,
                      "sample_over_commit": round(med["sample"] / med["commit"], 5)}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
