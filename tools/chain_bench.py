"""What the chain's bench tools share: the fixture lookup (every tool), and for bench_commit, bench_decommit, bench_sample,
bench_composition and bench_fri the command line, the chain of a fixture run up to the stage a tool times from, and the
interleaved HIP-event timing loop."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def add_args(ap, fixture, log_blowup):
    ap.add_argument("--fixture", default=fixture)
    ap.add_argument("--log-blowup", type=int, default=log_blowup)
    ap.add_argument("--proofs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--copies", type=int, default=1)


def open_fixture(args):
    """The package, and args.fixture with its PcsConfig and inputs from the manifest -> (rsv, proof, cfg, inputs)."""
    import rsvload
    rsv = rsvload.load_package()
    import bench
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        man = {e["file"]: e for e in json.load(f)["proofs"]}
    e = man[args.fixture]
    inputs = [(i, tuple(v)) for i, v in e["inputs"]]
    cfg = rsv.PcsConfig(e["pow_bits"], e["log_blowup_factor"], e["log_last_layer_degree_bound"], e["n_queries"])
    return rsv, bench.read_fixture(args.fixture), cfg, inputs


def open_chain(args, upto, caps=False, log_last=None):
    """The fixture's program (open_fixture, WitnessProgram.build), a Context, and a zero-filled Chain of args.proofs
    copies of the fixture run through the stage `upto` -> (rsv, ctx, wp, chain)."""
    rsv, proof, cfg, inputs = open_fixture(args)
    wp = rsv.WitnessProgram.build(proof, cfg, inputs, copies=args.copies)
    ctx = rsv.Context(0)
    chain = rsv.Chain(ctx, wp, args.proofs, args.log_blowup, log_last=log_last, caps=caps)
    chain.witness([proof] * args.proofs, inputs)
    stages = ("trace", "commit", "tree3", "sample", "fri")
    for stage in stages[:stages.index(upto) + 1]:
        getattr(chain, stage)()
    return rsv, ctx, wp, chain


def time_interleaved(ctx, calls, steps, warmup):
    """`warmup` rounds of every call, then `steps` rounds timed call by call with HIP events on the context's stream ->
    (times {name: [ms]}, medians {name: ms})."""
    import torch
    for _ in range(warmup):
        for call in calls.values():
            call()
    ctx.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.current_stream()
    times = {k: [] for k in calls}
    for _ in range(steps):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return times, {k: float(np.median(v)) for k, v in times.items()}
