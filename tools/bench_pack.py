#!/usr/bin/env python3
"""Time of the device serialiser (Chain.pack) beside the host path it replaces (Chain.proofs) and the FRI openings as the
scale, for 1 and 16 proofs of the same fixture interleaved in one process, one JSON line.

    python tools/bench_pack.py --fixture level10-1.bin --log-blowup 1 --log-last 0 --queries 16 --steps 9

Per batch size, `--steps` rounds after `--warmup`, medians in ms:
  pack         Chain.pack(): HIP events on the context's stream around the call (the blob's prefill on torch's stream
               included: the context waits for it);
  fri_open     Chain.fri_open(), the same way;
  pack_wall    Chain.pack() by the host's clock, from an idle device to the end of ctx.synchronize();
  pack_exact   Chain.pack(exact=True) by the host's clock likewise: the offsets-only call, the read of d_offsets[n], the
               exact allocation, the pack;
  proofs       Chain.proofs() by the host's clock: Chain.numpy() (synchronises, copies every chain tensor to the host),
               then proof_bytes per proof.
`bytes` is d_offsets[n], `bound` the blob Chain.pack() allocates."""
import argparse
import json
import time

import numpy as np

from chain_bench import add_args, open_chain


def main():
    import torch
    ap = argparse.ArgumentParser()
    add_args(ap, "level10-1.bin", 1)
    ap.add_argument("--log-last", type=int, default=0)
    ap.add_argument("--pow-bits", type=int, default=10)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    args = ap.parse_args()
    runs = {}
    for n in args.batches:
        args.proofs = n
        rsv, ctx, wp, ch = open_chain(args, "fri", caps=True, log_last=args.log_last)
        ch.pow(args.pow_bits, args.queries)
        ch.open()
        ch.fri_open()
        runs[n] = (ctx, wp, ch)

    def events(ctx, call):
        stream = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(ctx, call):
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    times = {n: {k: [] for k in ("pack", "fri_open", "pack_wall", "pack_exact", "proofs")} for n in runs}
    for step in range(args.warmup + args.steps):
        for n, (ctx, _, ch) in runs.items():
            got = {"pack": events(ctx, ch.pack), "fri_open": events(ctx, ch.fri_open), "pack_wall": wall(ctx, ch.pack),
                   "pack_exact": wall(ctx, lambda: ch.pack(exact=True)), "proofs": wall(ctx, ch.proofs)}
            if step >= args.warmup:
                for k, v in got.items():
                    times[n][k].append(v)
    out = {"tool": "bench_pack", "fixture": args.fixture, "log_blowup": args.log_blowup, "log_last": args.log_last, "queries": args.queries,
           "steps": args.steps, "batches": {}}
    for n, (ctx, wp, ch) in runs.items():
        blob, offsets = ch.pack()
        exact, _ = ch.pack(exact=True)
        ctx.synchronize()
        host = ch.proofs()
        total = int(offsets[n].item())
        same = blob[:total].cpu().numpy().tobytes() == exact.cpu().numpy().tobytes() == b"".join(p or b"" for p in host)
        out["batches"][str(n)] = {"bytes": total, "bound": blob.numel(), "same_as_host": bool(same),
                                  "ms": {k: round(float(np.median(v)), 4) for k, v in times[n].items()},
                                  "ms_all": {k: [round(t, 4) for t in v] for k, v in times[n].items()}}
        ctx.close()
        wp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
