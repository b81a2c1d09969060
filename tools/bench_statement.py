#!/usr/bin/env python3
"""The statement digest alone (rsv_statement_digest_dev) in both of its forms, beside the bare permutation's rate
(rsv_poseidon2_permute_dev on 2^24 resident states, as tools/perm_bench.py measures it) in the same session.  A group of T
value words costs S = ceil(T / 8) + 1 dependent permutations; the rate reported is n_groups * S permutations over the
median time of a call.  Times are HIP events on the context's stream around each call, the two forms interleaved
(tools/chain_bench.py).  One JSON line per (n_groups, T).

--eval-sizes adds the evaluating call (rsv_witness_eval_inputs_dev) with a hashed program beside the program that carries the
inner statement as a public input, on replicated S1 proofs.

    python tools/bench_statement.py [--cases 1:8,1024:8,65536:8,1:1024,1024:1024,65536:1024] [--steps 20] [--warmup 3]
                                    [--eval-sizes 1,1024,16384] [--downstream 16:64:4]

--downstream copies:n_own:groups times the chain behind the witness (trace() .. verify()) for the program that carries every
inner record as a public input beside the hashed one."""
import argparse
import json

import numpy as np

import chain_bench as CB

FORMS = {"row": (1 << 26) + 1, "lane": 1}    # statement_row_max: 1 + the largest batch hashed in the row form


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1:8,1024:8,65536:8,1:1024,1024:1024,65536:1024", help="n_groups:T, comma separated")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eval-sizes", default="", help="batch sizes of the evaluation comparison, e.g. 1,1024,16384 (empty: skipped)")
    ap.add_argument("--eval-steps", type=int, default=9)
    ap.add_argument("--downstream", default="", help="copies:n_own:groups of the downstream comparison, e.g. 16:64:4 (empty: skipped)")
    args = ap.parse_args()
    import torch
    import rsvload
    rsv = rsvload.load_package()
    if rsv.device_count() < 1:
        raise SystemExit("bench_statement needs a HIP device")
    dev = torch.device("cuda", 0)
    ctx = rsv.Context(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    m = 1 << 24
    d_in = torch.randint(0, 0x7FFFFFFF, (m, 16), dtype=torch.int32, device=dev, generator=gen)
    d_out = torch.empty_like(d_in)
    _, med = CB.time_interleaved(ctx, {"permute": lambda: ctx.poseidon2_permute(d_in, d_out)}, 5, 2)
    perm_rate = m / (med["permute"] * 1e-3)
    del d_in, d_out
    print(json.dumps({"permute_states": m, "ms_median": round(med["permute"], 4), "perms_per_s": round(perm_rate)}), flush=True)
    for case in args.cases.split(","):
        n, T = (int(x) for x in case.split(":"))
        copies = 1 if T <= 4096 else 64
        n_own = T // copies
        S = -(-T // 8) + 1
        d_rec = torch.zeros((n * copies, n_own, 5), dtype=torch.int32, device=dev)
        d_rec[:, :, 1] = torch.randint(0, 0x7FFFFFFF, (n * copies, n_own), dtype=torch.int32, device=dev, generator=gen)
        out = {f: (torch.zeros((n, 8, 5), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)) for f in FORMS}

        def call(form):
            def run():
                ctx.set_option("statement_row_max", FORMS[form])
                ctx.statement_digest(d_rec, n, copies, n_own, *out[form])
            return run

        times, med = CB.time_interleaved(ctx, {f: call(f) for f in FORMS}, args.steps, args.warmup)
        ctx.set_option("statement_row_max", 0)
        ctx.synchronize()
        same = torch.equal(out["row"][0], out["lane"][0]) and not out["row"][1].any().item() and not out["lane"][1].any().item()
        rate = {f: n * S / (med[f] * 1e-3) for f in FORMS}
        print(json.dumps({"n_groups": n, "T": T, "permutations_per_group": S, "steps": args.steps, "forms_equal": bool(same),
                          "ms_median": {f: round(v, 4) for f, v in med.items()},
                          "ms_min": {f: round(float(np.min(v)), 4) for f, v in times.items()},
                          "perms_per_s": {f: round(v) for f, v in rate.items()},
                          "fraction_of_permute": {f: round(v / perm_rate, 4) for f, v in rate.items()},
                          "input_bytes": n * T * 20}), flush=True)
        assert same, "the two forms differ"
        del d_rec, out
    if args.eval_sizes:
        eval_cost(rsv, ctx, torch, dev, args)
    if args.downstream:
        downstream(rsv, ctx, torch, dev, args)
    ctx.close()


def eval_cost(rsv, ctx, torch, dev, args):
    """rsv_witness_eval_inputs_dev on an S1 proof (tools/bench_witness_inputs.py's) replicated: the program with the fourth
    record a public input of the outer circuit beside the hashed program of the same proof — the cost of the S extra
    invocations and of the digest launch.  One JSON line per batch size."""
    import bench_witness_inputs as BW
    proof, cfg, inputs = BW.s1_proof(rsv, ctx)
    plain = rsv.WitnessProgram.build(proof, cfg, inputs, n_fixed=3)
    hashed = rsv.WitnessProgram.build(proof, cfg, inputs, n_fixed=3, hashed=True)
    rec = np.array([[k] + list(v) for k, v in inputs[3:]], dtype=np.uint32).reshape(1, 1, 5)
    for n in (int(x) for x in args.eval_sizes.split(",")):
        blob, offsets = rsv.pack([proof] * n)
        d_blob, d_offsets = torch.from_numpy(blob.copy()).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)
        d_inputs = torch.from_numpy(rec.view(np.int32)).to(dev).repeat(n, 1, 1).contiguous()
        out = {k: (torch.zeros((n, p.n_vars, 4), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))
               for k, p in (("own_inputs", plain), ("hashed", hashed))}
        calls = {"own_inputs": lambda: ctx.witness(plain, d_blob, d_offsets, n, *out["own_inputs"], inputs=inputs[:3], d_inputs=d_inputs),
                 "hashed": lambda: ctx.witness(hashed, d_blob, d_offsets, n, *out["hashed"], inputs=inputs[:3], d_inputs=d_inputs)}
        times, med = CB.time_interleaved(ctx, calls, args.eval_steps, args.warmup)
        ctx.synchronize()
        assert all(int(v[1].sum().item()) == n for v in out.values())
        print(json.dumps({"eval": "S1", "proofs": n, "steps": args.eval_steps, "n_vars": {k: int(v[0].shape[1]) for k, v in out.items()},
                          "num_input": {"own_inputs": plain.num_input, "hashed": hashed.num_input},
                          "ms_median": {k: round(v, 4) for k, v in med.items()},
                          "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
                          "hashed_over_own_inputs": round(med["hashed"] / med["own_inputs"], 4)}), flush=True)
        del d_blob, d_offsets, d_inputs, out
    plain.close()
    hashed.close()


def downstream(rsv, ctx, torch, dev, args):
    """What the statement's size costs behind the witness: groups of `copies` proofs with n_own own records each (an S1
    circuit with 3 + n_own public inputs, proved here, one proof replicated) through the program that carries every record
    (num_input = 3 + copies * n_own) and through the hashed one (11); every stage of the chain from trace() to verify() timed
    on the host around a synchronisation, the median of --eval-steps runs.  One JSON line per program."""
    import time
    sys_path_tests()
    from tests import verify_inputs_ref as V
    copies, n_own, groups = (int(x) for x in args.downstream.split(":"))
    cfg = rsv.PcsConfig(3, 1, 0, 9)
    proof = None
    for seed in range(1, 9):
        b = V.build_many(3 + n_own, first=11, seed=seed)
        circ = rsv.Circuit(b.gates, b.flow_wires, b.n_vars, 3 + n_own, b.witness_ops)
        ch = rsv.Chain(ctx, circ, 1, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, caps=True)
        ch.load(b.variables[None], b.unbound_flow()[None])
        finish(ch, cfg)
        one = ch.proofs()[0]
        circ.close()
        if one is not None and rsv.verify_batch([one], cfg, b.inputs)[0][0]:
            proof, inputs = one, b.inputs
            break
    if proof is None:
        raise SystemExit("no inner proof verified")
    rec = np.array([[k] + list(v) for k, v in inputs[3:]], dtype=np.uint32).reshape(1, n_own, 5)
    members = groups * copies
    blob, offsets = rsv.pack([proof] * members)
    pair = (torch.from_numpy(blob.copy()).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev))
    d_own = torch.from_numpy(rec.view(np.int32)).to(dev).repeat(members, 1, 1).contiguous()
    stages = ("witness", "trace", "commit", "tree3", "sample", "fri", "pow", "open", "fri_open", "verify")
    for name, hashed in (("own_inputs", False), ("hashed", True)):
        t0 = time.perf_counter()
        wp = rsv.WitnessProgram.build(proof, cfg, inputs, copies=copies, n_fixed=3, hashed=hashed)
        build_s = time.perf_counter() - t0
        runs = {st: [] for st in stages}
        for _ in range(args.eval_steps + 1):
            ch = rsv.Chain(ctx, wp, groups, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, caps=True, aggregate=True)
            for st in stages:
                ctx.synchronize()
                t0 = time.perf_counter()
                if st == "witness":
                    ch.witness(pair, inputs[:3], d_inputs=d_own)
                elif st == "pow":
                    ch.pow(cfg.pow_bits, cfg.n_queries)
                elif st == "verify":
                    acc, reason = ch.verify(cfg)
                else:
                    getattr(ch, st)()
                ctx.synchronize()
                runs[st].append((time.perf_counter() - t0) * 1e3)
        med = {st: float(np.median(v[1:])) for st, v in runs.items()}  # (the first run uploads the program's tables)
        print(json.dumps({"downstream": name, "copies": copies, "n_own": n_own, "groups": groups, "num_input": wp.num_input, "n_vars": wp.n_vars,
                          "log_sizes": list(wp.trace_sizes()), "build_s": round(build_s, 2), "steps": args.eval_steps,
                          "accepted": int(acc.sum().item()), "reasons": reason.cpu().tolist(),
                          "ms_median": {st: round(v, 3) for st, v in med.items()},
                          "ms_trace_to_verify": round(sum(v for st, v in med.items() if st != "witness"), 3)}), flush=True)
        wp.close()


def finish(ch, cfg):
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch, stage)()
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.open()
    ch.fri_open()


def sys_path_tests():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)


if __name__ == "__main__":
    main()
