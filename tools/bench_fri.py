#!/usr/bin/env python3
"""Time of the commit phase of FRI of the next proof beside the commitment of trees 0-2 of the same proof in the same run,
one JSON line.

    python tools/bench_fri.py --fixture level10-1.bin --log-blowup 1 --log-last 0 --proofs 16 --steps 5

Timed interleaved, `--steps` rounds, HIP events on the context's stream, medians:
  commit       rsv_witness_commit_dev on the chain's buffers (the yardstick: its forward FFT of the 126 columns is what
               the quotient call does again);
  fri          rsv_witness_fri_dev on what tree 3 and the sampling left (the channel is restored before every call):
               the sample mixes, the quotient columns and the layers;
  fri_commit   rsv_fri_commit_dev alone on the quotient columns that call left;
  fri_commit_cap  with `--sub-log h` (1 .. 8): rsv_fri_commit_cap_dev on the same columns in the same rounds, leaving the caps
               of the layer trees (the same launches: the kept levels are written where they stay);
  fri_commit_tail  with `--tail-log t` (1 .. 10): rsv_fri_commit_tail_dev on the same columns in the same rounds, the tail form
               (fewer launches, the same outputs); with `--sub-log` it also leaves the caps;
  fri_tail     with `--tail-log t`: rsv_witness_fri_tail_dev, `fri` end to end with the commit phase in the tail form.
`quotients` is fri - fri_commit.  The shares of the row kernel (k_fr_rows), the extension (k_cm_fft_*), the layer trees
(k_fr_hash_layer), the folds (k_fr_fold) and the channel steps (k_fr_draw) are the rows of
`rocprofv3 --kernel-trace --stats -- python tools/bench_fri.py ...`."""
import argparse
import json

from chain_bench import add_args, open_chain, time_interleaved


def main():
    ap = argparse.ArgumentParser()
    add_args(ap, "level10-1.bin", 1)
    ap.add_argument("--log-last", type=int, default=0)
    ap.add_argument("--sub-log", type=int, default=0)
    ap.add_argument("--tail-log", type=int, default=0)
    args = ap.parse_args()
    rsv, ctx, wp, ch = open_chain(args, "sample", log_last=args.log_last)
    import torch
    lp, lq, n, b = ch.lp, ch.lq, ch.n, ch.log_blowup
    sz = rsv.fri_sizes(lp, lq, b, args.log_last)
    ni = sz["n_inner"]
    chan0, ch.channel = ch.channel, torch.zeros_like(ch.channel)  # what tree 3 left: every fri() starts from a copy of it

    def fri():
        ch.channel.copy_(chan0)
        ch.fri()

    calls = {
        "commit": ch.commit,
        "fri": fri,
        "fri_commit": lambda: ctx.fri_commit(ch.quot, sz["sizes"], b, args.log_last, n, ch.channel, ch.fri_roots, ch.alphas, ch.layers,
                                             ch.last_poly, ch.low_degree, d_mask=ch.ok),
    }
    extra = {}
    if args.sub_log:
        cap_words = rsv.fri_cap_sizes(sz["sizes"], b, args.log_last, args.sub_log, n)[0]
        caps = torch.zeros(max(cap_words, 1), dtype=torch.int32, device=ch.device)
        calls["fri_commit_cap"] = lambda: ctx.fri_commit(ch.quot, sz["sizes"], b, args.log_last, n, ch.channel, ch.fri_roots, ch.alphas, ch.layers,
                                                         ch.last_poly, ch.low_degree, d_mask=ch.ok, sub_log=args.sub_log, d_caps=caps)
        extra = {"sub_log": args.sub_log, "cap_words": cap_words}
    if args.tail_log:
        tail_caps = torch.zeros_like(caps) if args.sub_log else None
        calls["fri_commit_tail"] = lambda: ctx.fri_commit(ch.quot, sz["sizes"], b, args.log_last, n, ch.channel, ch.fri_roots, ch.alphas, ch.layers,
                                                          ch.last_poly, ch.low_degree, d_mask=ch.ok, sub_log=args.sub_log, d_caps=tail_caps,
                                                          tail_log=args.tail_log)

        def fri_tail():
            ch.fri_tail_log = args.tail_log
            fri()
            ch.fri_tail_log = 0

        calls["fri_tail"] = fri_tail
        extra["tail_log"] = args.tail_log
    times, med = time_interleaved(ctx, calls, args.steps, max(args.warmup, 1))
    if args.sub_log:
        extra["commit_cap_over_fri_commit"] = round(med["fri_commit_cap"] / med["fri_commit"], 5)
    if args.tail_log:
        extra["commit_tail_over_fri_commit"] = round(med["fri_commit_tail"] / med["fri_commit"], 5)
    ok = int(ch.ok.sum().item())
    positions = sum(1 << s for s in sz["sizes"])
    print(json.dumps({"tool": "bench_fri", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "sizes": sz["sizes"], "n_inner": ni,
                      "log_blowup": b, "log_last": args.log_last, "proofs": n, "ok": ok, "low_degree": int(ch.low_degree.sum().item()),
                      "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
                      "quotients_ms": round(med["fri"] - med["fri_commit"], 4), "fri_over_commit": round(med["fri"] / med["commit"], 5),
                      "quotient_positions_per_proof": positions, **extra}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
