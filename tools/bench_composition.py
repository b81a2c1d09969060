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

import numpy as np
from chain_bench import add_args, open_chain, time_interleaved


def main():
    ap = argparse.ArgumentParser()
    add_args(ap, "level10-1.bin", 1)
    args = ap.parse_args()
    rsv, ctx, wp, ch = open_chain(args, "commit")
    import torch
    lp, lq, n, b = ch.lp, ch.lq, ch.n, ch.log_blowup
    L3 = rsv.composition_log_size(lp, lq)
    ppre, qpre = wp.preprocessed()
    d_ppre = torch.from_numpy(np.ascontiguousarray(ppre, dtype=np.uint32).view(np.int32)).to(ch.device)
    d_qpre = torch.from_numpy(np.ascontiguousarray(qpre, dtype=np.uint32).view(np.int32)).to(ch.device)
    chan0 = ch.channel.clone()  # what the commitment left: every tree3() starts from it

    def tree3():
        ch.channel.copy_(chan0)
        ch.tree3()

    calls = {
        "commit": ch.commit,
        "tree3": tree3,
        "composition": lambda: ctx.composition(lp, lq, (d_ppre, ch.plonk, ch.int_plonk), (d_qpre, ch.poseidon, ch.int_poseidon), ch.sums,
                                               ch.draws, n, ch.comp, d_mask=ch.ok),
    }
    times, med = time_interleaved(ctx, calls, args.steps, max(args.warmup, 1))
    ok = int(ch.ok.sum().item())
    print(json.dumps({"tool": "bench_composition", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "log_composition": L3,
                      "log_blowup": b, "proofs": n, "ok": ok, "ms": {k: round(v, 4) for k, v in med.items()},
                      "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
                      "tree3_over_commit": round(med["tree3"] / med["commit"], 5),
                      "composition_over_tree3": round(med["composition"] / med["tree3"], 5)}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
