#!/usr/bin/env python3
"""rsv_witness_eval_dev (the statement a constant of the program) beside rsv_witness_eval_inputs_dev (every proof its own
statement, here the same one replicated) in one session, for two shapes:

  small   small_proof.bin under the program rsv_witness_program_build makes, both calls on that program: n_own = 0, where the
          new call has to be the old one;
  s1      a proof of circuit S1 (tests/user_circuit_ref.py) under (3, 1, 0, 9), the smallest the project proves, made here
          by the chain: the old call on the program with the statement a constant, the new call on the program with the
          fourth record the proof's own (n_own = 1).

Times are HIP events on the context's stream around each call, interleaved (tools/chain_bench.py), in both orders of the
two calls.  One JSON line per (shape, proofs, order).

--baseline-only times rsv_witness_eval_dev alone and uses nothing this change added, so that the same file runs in a
checkout of the commit before it, against that commit's library.

    python tools/bench_witness_inputs.py [--shapes small,s1] [--sizes 1,64,1024] [--steps 9] [--warmup 3] [--baseline-only]"""
import argparse
import json

import numpy as np

import chain_bench as CB

S1_CONFIG = (3, 1, 0, 9)


def s1_proof(rsv, ctx):
    """One proof of S1 that verifies (a witness whose proof draws a query position twice is made again), its inputs."""
    from tests import circuit_eval_ref as E
    cfg = rsv.PcsConfig(*S1_CONFIG)
    for seed in range(1, 9):
        b = E.build("S1", pub=(11, 0, 0, 0), seed=seed, bit=1)
        circ = rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, **E.create_args(b))
        ch = rsv.Chain(ctx, circ, 1, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, caps=True)
        ch.evaluate(E.inputs_of(b)[None], E.flow_in_of(b)[None], check=True)
        for stage in ("trace", "commit", "tree3", "sample", "fri"):
            getattr(ch, stage)()
        ch.pow(cfg.pow_bits, cfg.n_queries)
        ch.open()
        ch.fri_open()
        proof = ch.proofs()[0]
        circ.close()
        if proof is not None and rsv.verify_batch([proof], cfg, b.inputs)[0][0]:
            return proof, cfg, b.inputs
    raise SystemExit("no S1 proof verified")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,s1")
    ap.add_argument("--sizes", default="1,64,1024")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    import torch
    ap2 = argparse.Namespace(fixture="small_proof.bin")
    rsv, small, small_cfg, small_inputs = CB.open_fixture(ap2)
    if rsv.device_count() < 1:
        raise SystemExit("bench_witness_inputs needs a HIP device")
    dev = torch.device("cuda", 0)
    ctx = rsv.Context(0)
    for shape in args.shapes.split(","):
        if shape == "small":
            proof, cfg, inputs, n_own = small, small_cfg, small_inputs, 0
        else:
            proof, cfg, inputs = s1_proof(rsv, ctx)
            n_own = 1
        n_fixed = len(inputs) - n_own
        constant = rsv.WitnessProgram.build(proof, cfg, inputs)
        own = None if args.baseline_only else (constant if n_own == 0 else rsv.WitnessProgram.build(proof, cfg, inputs, n_fixed=n_fixed))
        rec = np.array([[k] + list(v) for k, v in inputs[n_fixed:]], dtype=np.uint32).reshape(1, n_own, 5)
        for n in (int(x) for x in args.sizes.split(",")):
            blob, offsets = rsv.pack([proof] * n)
            d_blob, d_offsets = torch.from_numpy(blob.copy()).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)
            d_inputs = torch.from_numpy(rec.view(np.int32)).to(dev).repeat(n, 1, 1).contiguous()
            out = {k: (torch.zeros((n, p.n_vars, 4), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))
                   for k, p in (("constant", constant), ("inputs", own)) if p is not None}
            calls = {"constant": lambda: ctx.witness(constant, d_blob, d_offsets, n, *out["constant"], inputs=inputs)}
            if own is not None:
                calls["inputs"] = lambda: ctx.witness(own, d_blob, d_offsets, n, *out["inputs"], inputs=inputs[:n_fixed], d_inputs=d_inputs)
            for order in ("constant_first", "inputs_first"):
                if order == "inputs_first":
                    if own is None:
                        continue
                    calls = dict(reversed(list(calls.items())))
                times, med = CB.time_interleaved(ctx, calls, args.steps, args.warmup)
                ctx.synchronize()
                accepted = {k: int(v[1].sum().item()) for k, v in out.items()}
                assert all(a == n for a in accepted.values()), accepted
                if own is not None and n_own == 0:
                    assert torch.equal(out["constant"][0], out["inputs"][0]), "n_own = 0: the two calls' variables differ"
                print(json.dumps({"shape": shape, "proofs": n, "n_own": n_own, "order": order, "steps": args.steps,
                                  "n_vars": {k: int(v[0].shape[1]) for k, v in out.items()},
                                  "ms_median": {k: round(v, 4) for k, v in med.items()},
                                  "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
                                  "ms_max": {k: round(float(np.max(v)), 4) for k, v in times.items()},
                                  "inputs_over_constant": None if own is None else round(med["inputs"] / med["constant"], 4)}), flush=True)
            del d_blob, d_offsets, d_inputs, out
        if own is not None and own is not constant:
            own.close()
        constant.close()
    ctx.close()


if __name__ == "__main__":
    main()
