#!/usr/bin/env python3
"""Time of the openings of the FRI layer trees of the next proof (Chain.fri_open) beside the commitment of trees 0-2, the
commit phase of FRI and its layer part alone, of the same proof in the same run, one JSON line.

    python tools/bench_fri_open.py --fixture level10-1.bin --log-blowup 1 --log-last 0 --queries 16 --proofs 1 --steps 5

Timed interleaved, `--steps` rounds, HIP events on the context's stream, medians:
  commit       rsv_witness_commit_dev on the chain's buffers (the yardstick of the other chain tools);
  fri          rsv_witness_fri_dev (the channel is restored before every call);
  fri_commit   rsv_fri_commit_dev alone on the quotient columns that call left: the layer trees, the folds and the channel
               steps (from whatever channel the call before left: its time does not depend on the words).  The opening
               hashes the same trees again, so this is what it is read against;
  fri_open     rsv_fri_open_dev at the positions drawn once from the channel fri left (pow_bits as given).
With `--sub-log h` (1 .. 8) the cap forms run in the same rounds, behind the forms above:
  fri_commit_cap  rsv_fri_commit_cap_dev on the same columns, leaving the caps of the layer trees (same launches);
  fri_open_cap    rsv_fri_open_cap_dev from those caps at the same positions (six launches); `cap_equal` says that its four
                  outputs equal rsv_fri_open_dev's on the same layers, word for word.
`launches` counts what one opening enqueues: per tree a hash launch a level and a gather every second level, and the zero,
the plan and the value gather.  For a per-kernel split run the tool under
`rocprofv3 --kernel-trace --stats -- python tools/bench_fri_open.py ...`."""
import argparse
import json

from chain_bench import add_args, open_chain, time_interleaved


def main():
    ap = argparse.ArgumentParser()
    add_args(ap, "level10-1.bin", 1)
    ap.add_argument("--log-last", type=int, default=0)
    ap.add_argument("--pow-bits", type=int, default=10)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--sub-log", type=int, default=0)
    args = ap.parse_args()
    rsv, ctx, wp, ch = open_chain(args, "sample", log_last=args.log_last)
    lp, lq, n, b = ch.lp, ch.lq, ch.n, ch.log_blowup
    sz = rsv.fri_sizes(lp, lq, b, args.log_last)
    M, ni = sz["sizes"][0], sz["n_inner"]
    ctx.release_to_torch()  # the copies below run on torch's stream: behind the context's work
    chan_tree3 = ch.channel.clone()
    ch.fri()
    ch.pow(args.pow_bits, args.queries)
    ch.fri_open()

    def restored(chan, call):
        def run():
            ctx.release_to_torch()
            ch.channel.copy_(chan)
            call()
        return run

    calls = {
        "commit": ch.commit,
        "fri": restored(chan_tree3, ch.fri),
        "fri_commit": lambda: ctx.fri_commit(ch.quot, sz["sizes"], b, args.log_last, n, ch.channel, ch.fri_roots, ch.alphas, ch.layers,
                                             ch.last_poly, ch.low_degree, d_mask=ch.ok),
        "fri_open": ch.fri_open,
    }
    h, extra = args.sub_log, {}
    if h:
        import torch
        cap_words = rsv.fri_cap_sizes(sz["sizes"], b, args.log_last, h, n)[0]
        caps = torch.zeros(max(cap_words, 1), dtype=torch.int32, device=ch.device)
        calls["fri_commit_cap"] = lambda: ctx.fri_commit(ch.quot, sz["sizes"], b, args.log_last, n, ch.channel, ch.fri_roots, ch.alphas, ch.layers,
                                                         ch.last_poly, ch.low_degree, d_mask=ch.ok, sub_log=h, d_caps=caps)
        outs = (ch.fri_witness, ch.n_fri_witness, ch.fri_hash_witness, ch.n_fri_hash_witness)
        calls["fri_open_cap"] = lambda: ctx.fri_open(ch.quot, ch.layers, sz["sizes"], b, args.log_last, n, ch.queries, args.queries, *outs,
                                                     d_mask=ch.ok, sub_log=h, d_caps=caps)
    times, med = time_interleaved(ctx, calls, args.steps, max(args.warmup, 1))
    if h:
        # the layers are the last capped commitment's: the recompute form on them, then the cap form again
        ch.fri_open()
        ctx.release_to_torch()
        want = [t.clone() for t in outs]
        for t in outs:
            t.fill_(-1)
        calls["fri_open_cap"]()
        ctx.release_to_torch()
        extra = {"sub_log": h, "cap_words": cap_words, "cap_equal": all(bool(torch.equal(a, w)) for a, w in zip(outs, want)),
                 "open_cap_over_open": round(med["fri_open_cap"] / med["fri_open"], 5),
                 "commit_cap_over_fri_commit": round(med["fri_commit_cap"] / med["fri_commit"], 5), "launches_cap": 6}
    got = ch.numpy()
    levels = sum(M - t for t in range(1 + ni))
    print(json.dumps({"tool": "bench_fri_open", "fixture": args.fixture, "log_plonk": lp, "log_poseidon": lq, "sizes": sz["sizes"], "n_inner": ni,
                      "log_blowup": b, "log_last": args.log_last, "queries": args.queries, "proofs": n, "ok": int(got["ok"].sum()),
                      "n_fri_witness": got["n_fri_witness"][0].tolist(), "n_hash_witness": got["n_fri_hash_witness"][0].tolist(),
                      "capacities": list(rsv.fri_open_sizes(sz["sizes"], b, args.log_last, args.queries)),
                      "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
                      "open_minus_fri_commit_ms": round(med["fri_open"] - med["fri_commit"], 4),
                      "open_over_fri_commit": round(med["fri_open"] / med["fri_commit"], 5),
                      "launches": {"hash": levels, "gather": sum((M - t + 1) // 2 for t in range(1 + ni)), "other": 3}, **extra}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
