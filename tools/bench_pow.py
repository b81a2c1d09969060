#!/usr/bin/env python3
"""Time of the proof of work and the query draw of the next proof (Chain.pow) and of the openings of trees 0-3 at the drawn
positions (Chain.open) beside the commitment of trees 0-2 and the commit phase of FRI of the same proof in the same run, with
the search's candidate rate beside the bare permutation kernel's in the same session, one JSON line.

    python tools/bench_pow.py --fixture level10-1.bin --log-blowup 1 --log-last 0 --pow-bits 20 --proofs 1 --steps 5

Timed interleaved, `--steps` rounds, HIP events on the context's stream, medians:
  commit       rsv_witness_commit_caps_dev on the chain's buffers (the yardstick of the other chain tools);
  fri          rsv_witness_fri_dev (the channel is restored before every call);
  pow          rsv_pow_grind_dev + rsv_draw_queries_dev from the channel fri left (channel and ok restored before every call);
  open         rsv_witness_decommit_dev with caps + rsv_decommit_tree_dev of tree 3 with its cap, at the drawn positions;
  exhaust      rsv_pow_grind_dev at RSV_MAX_POW_BITS over exactly `--exhaust` candidates per proof from the same channel: a
               search that (but for a chance hit, reported) tests every candidate, so candidates / time is the kernel's
               sustained rate with no over-search in it;
  permute      rsv_poseidon2_permute_dev on 2^24 states (tools/perm_bench.py's shape): the k_permute rate.
The search's candidates are counted as the found nonce + 1 per proof (`search_rate`); what the search tested beyond them is
estimated as pow-time x exhaust rate - candidates (`over_search_estimate`: it also holds the launches, the finish and the draw
kernels, so it is an upper estimate) beside the bound, the lanes of one round (`round_lanes`).  `model_ceiling` is
tools/perm_ceiling.py's instruction-cost ceiling of the full permutation.  For a per-kernel split run the tool under
`rocprofv3 --kernel-trace --stats -- python tools/bench_pow.py ...`."""
import argparse
import json

from chain_bench import add_args, open_chain, time_interleaved
from perm_ceiling import ceiling


def main():
    ap = argparse.ArgumentParser()
    add_args(ap, "level10-1.bin", 1)
    ap.add_argument("--log-last", type=int, default=0)
    ap.add_argument("--pow-bits", type=int, default=20)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--exhaust", type=int, default=1 << 26)
    ap.add_argument("--log-states", type=int, default=24)
    args = ap.parse_args()
    rsv, ctx, wp, ch = open_chain(args, "sample", caps=True, log_last=args.log_last)
    import torch
    n = ch.n
    ctx.release_to_torch()  # the copies below run on torch's stream: behind the context's work
    chan_tree3 = ch.channel.clone()
    ch.fri()
    ctx.release_to_torch()
    chan_fri, ok0 = ch.channel.clone(), ch.ok.clone()
    x_chan, x_ok, x_nonce = chan_fri.clone(), ok0.clone(), torch.zeros((n, 2), dtype=torch.int32, device=ch.device)
    gen = torch.Generator(device=ch.device)
    gen.manual_seed(1)
    d_in = torch.randint(0, 0x7FFFFFFF, (1 << args.log_states, 16), dtype=torch.int32, device=ch.device, generator=gen)
    d_out = torch.empty_like(d_in)

    def fri():
        ctx.release_to_torch()
        ch.channel.copy_(chan_tree3)
        ch.fri()

    def pow_():
        ctx.release_to_torch()
        ch.channel.copy_(chan_fri)
        ch.ok.copy_(ok0)
        ch.pow(args.pow_bits, args.queries)

    def exhaust():
        ctx.release_to_torch()
        x_chan.copy_(chan_fri)
        x_ok.copy_(ok0)
        ctx.pow_grind(30, n, x_ok, x_chan, x_nonce, max_tries=args.exhaust)

    calls = {"commit": ch.commit, "fri": fri, "pow": pow_, "open": ch.open, "exhaust": exhaust,
             "permute": lambda: ctx.poseidon2_permute(d_in, d_out)}
    times, med = time_interleaved(ctx, calls, args.steps, max(args.warmup, 1))
    got = ch.numpy()
    ok = int(ok0.sum().item())
    nonces = [int(lo) | int(hi) << 32 for lo, hi in got["nonce"].tolist()]
    candidates = sum(v + 1 for v, k in zip(nonces, got["ok"].tolist()) if k)
    exhausted = ok - int(x_ok.sum().item())
    exhaust_rate = exhausted * args.exhaust / (med["exhaust"] * 1e-3) if exhausted else 0.0
    search_rate = candidates / (med["pow"] * 1e-3)
    permute_rate = (1 << args.log_states) / (med["permute"] * 1e-3)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row_blocks = max(min(-(-(1 << args.pow_bits) // 256), max(cus * 8 // n, 1)), 1)  # pow_api.inc: pow_row_blocks
    print(json.dumps({"tool": "bench_pow", "fixture": args.fixture, "log_plonk": ch.lp, "log_poseidon": ch.lq, "log_blowup": ch.log_blowup,
                      "log_last": args.log_last, "pow_bits": args.pow_bits, "queries": args.queries, "proofs": n, "ok": ok,
                      "found": int(got["ok"].sum()), "nonces": nonces[:4], "candidates": candidates,
                      "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
                      "pow_over_commit": round(med["pow"] / med["commit"], 5), "open_over_commit": round(med["open"] / med["commit"], 5),
                      "search_rate": round(search_rate), "exhaust_candidates": args.exhaust, "exhaust_proofs_exhausted": exhausted,
                      "exhaust_rate": round(exhaust_rate), "permute_rate": round(permute_rate), "model_ceiling": round(ceiling()[0]),
                      "exhaust_over_permute": round(exhaust_rate / permute_rate, 4), "search_over_permute": round(search_rate / permute_rate, 4),
                      "over_search_estimate": round(med["pow"] * 1e-3 * exhaust_rate - candidates) if exhausted else None,
                      "round_lanes": row_blocks * 256 * ok}))
    ctx.close()
    wp.close()


if __name__ == "__main__":
    main()
