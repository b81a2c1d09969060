"""A caller's own circuit through the chain (`-m gpu`): rsv.Circuit, Context.circuit_check / circuit_flow, Chain.load.

1-3 run the level10-1 -> level11-1 pair's recursion circuit as a CREATED program: its gate list, flow wires and witness ops
given back to rsv_circuit_program_create with the variables and the flow the built program's witness() left, which pins the
created path to the reference (level11-1.bin byte for byte) and gives both device checks a circuit of 40 485 rows and 3 782
invocations.  4 and 5 run the three small circuits of tests/user_circuit_ref.py, whose shapes (lp + 2 != lq + 3, below 2^15
rows) no fixture has, against the oracle's columns and both verifiers.  Every expected index is the numpy model's
(tests/user_circuit_ref.py), which tests/test_user_circuit_host.py ties to the oracle's own two checks."""
import numpy as np
import pytest

from tests import interaction_ref as R
from tests import oracle_binding as ob
from tests import user_circuit_ref as U
from tests.chain_harness import DEV, FILL, chain, dev, inputs_of, pin_of, program_of, u32
from tests.conftest import fixture_cfg, read_proof
from tests.verify_grid import _finish, _run

pytestmark = pytest.mark.gpu
SRC, DST = "level10-1.bin", "level11-1.bin"
NONE = U.NONE
# (pow_bits, log_blowup, log_last, n_queries): both are within rsv_fri_sizes for all three shapes
CONFIGS = [(3, 1, 0, 9), (8, 2, 2, 16)]


@pytest.fixture(scope="module")
def ctx(rsv):
    c = rsv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def level10(rsv, ctx):
    """The built program of the pair, what its witness() left for one proof (host copies), and the created twin."""
    wp = program_of(rsv, pin_of(SRC))
    ch = chain(rsv, ctx, wp, [read_proof(SRC)], inputs_of(SRC), 1, upto="witness")
    ctx.synchronize()
    assert ch.acc.cpu().tolist() == [1]
    variables, flow, swap = u32(ch._vars)[0].copy(), u32(ch._flow)[0].copy(), ch._swap.cpu().numpy()[0].copy()
    gates, ops = wp.gates()
    wires = np.ascontiguousarray(wp.export().flow_wires, dtype=np.uint32)
    circ = rsv.Circuit(gates, wires, wp.n_vars, 3, ops)
    yield {"wp": wp, "circ": circ, "vars": variables, "flow": flow, "swap": swap, "gates": gates, "ops": ops, "wires": wires}
    circ.close()
    wp.close()


# ---------------------------------------------------------------- 1. the created program is the built one
def test_created_program_gives_the_next_fixture(rsv, ctx, level10):
    want, cfg = read_proof(DST), fixture_cfg(DST)
    circ = level10["circ"]
    assert circ.trace_sizes() == level10["wp"].trace_sizes() and circ.shape.flow_count == len(level10["wires"])
    ch = rsv.Chain(ctx, circ, 1, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, device=DEV)
    with pytest.raises(ValueError):
        ch.witness([read_proof(SRC)], inputs_of(SRC))
    with pytest.raises(ValueError):
        rsv.Chain(ctx, circ, 1, 1, aggregate=True)
    ch.load(level10["vars"][None], level10["flow"][None], level10["swap"][None])
    _finish(ch, cfg)
    a = ch.numpy()
    assert a["acc"].tolist() == [1] and a["bad_row"].tolist() == [NONE] and a["bad_flow"].tolist() == [NONE] and a["ok"].tolist() == [1]
    assert ch.proofs()[0] == want
    blob, offsets = ch.pack(exact=True)
    assert offsets.cpu().tolist() == [0, len(want)] and blob.cpu().numpy().tobytes() == want


# ---------------------------------------------------------------- 2. circuit_flow
def _flow(ctx, prog, variables, flow_in, ok=None):
    import torch
    n = len(variables)
    d_vars, d_flow = dev(variables), dev(flow_in)
    d_swap = torch.full(flow_in.shape[:2], 7, dtype=torch.uint8, device=DEV)
    d_ok = torch.ones(n, dtype=torch.uint8, device=DEV) if ok is None else torch.from_numpy(np.asarray(ok, np.uint8)).to(DEV)
    d_bad = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    ctx.circuit_flow(prog, d_vars, n, d_flow, d_swap, d_ok, d_bad)
    ctx.synchronize()
    return u32(d_flow), d_swap.cpu().numpy(), d_ok.cpu().numpy(), u32(d_bad)


def test_circuit_flow_restores_the_verifying_pass_flow(rsv, ctx, level10):
    """Every wire-bound half, every output and the swap bytes cleared: the call restores the verifying pass's flow word for
    word; with one bound output variable changed, bad_flow is the model's index.  The built program takes the call too."""
    v, flow, wires, gates = level10["vars"], level10["flow"], level10["wires"], level10["gates"]
    cleared = flow.copy()
    cleared[:, 16:] = 0
    for h in range(2):
        cleared[wires[:, h] != 0, 8 * h:8 * h + 8] = 0
    assert (wires[:, :2] == 0).any() and (wires[:, :2] != 0).any() and (wires[:, 4] != 0).any() and level10["swap"].any()
    want_bad, want_flow, want_swap = U.model_flow(gates, wires, v, cleared)
    assert want_bad == NONE and np.array_equal(want_flow, flow) and np.array_equal(want_swap, level10["swap"])
    for prog in (level10["circ"], level10["wp"]):
        got, swap, ok, bad = _flow(ctx, prog, v[None], cleared[None])
        assert ok.tolist() == [1] and bad.tolist() == [NONE]
        assert np.array_equal(got[0], flow) and np.array_equal(swap[0], level10["swap"])
    bound = np.flatnonzero(wires[:, 2] != 0)
    k = int(bound[len(bound) // 2])
    row = int(np.flatnonzero(gates[:, 4] == wires[k, 2])[0])
    tampered = v.copy()
    tampered[gates[row, 1], 2] ^= 1
    want_bad = U.model_flow(gates, wires, tampered, cleared)[0]
    assert want_bad != NONE and want_bad <= k
    free = np.stack([cleared, cleared, cleared])
    free[2, int(np.flatnonzero(wires[:, 0] == 0)[0]), 3] = U.P            # a word of a half without a wire set to P
    want_p = U.model_flow(gates, wires, v, free[2])[0]
    got, swap, ok, bad = _flow(ctx, level10["circ"], np.stack([tampered, v, v]), free)
    assert ok.tolist() == [0, 1, 0] and bad.tolist() == [want_bad, NONE, want_p] and want_p != NONE
    assert np.array_equal(got[1], flow) and np.array_equal(swap[1], level10["swap"])
    # a proof masked on entry: zero records, bad_flow all ones, ok stays 0
    got, swap, ok, bad = _flow(ctx, level10["circ"], np.stack([v, v]), np.stack([cleared, cleared]), ok=[0, 1])
    assert ok.tolist() == [0, 1] and bad.tolist() == [NONE, NONE] and not got[0].any() and not swap[0].any()
    assert np.array_equal(got[1], flow)


# ---------------------------------------------------------------- 3. circuit_check
def _check(ctx, prog, variables, by_variable, ok=None):
    import torch
    n = len(variables)
    d_vars = dev(np.ascontiguousarray(variables.transpose(1, 0, 2)) if by_variable else variables)
    d_ok = torch.ones(n, dtype=torch.uint8, device=DEV) if ok is None else torch.from_numpy(np.asarray(ok, np.uint8)).to(DEV)
    d_bad = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    ctx.circuit_check(prog, d_vars, n, d_ok, d_bad)
    ctx.synchronize()
    return d_ok.cpu().numpy(), u32(d_bad)


def _tampered(level10):
    """name -> (variables, the model's first failing row)."""
    v, gates, ops = level10["vars"], level10["gates"], level10["ops"]
    hint = int(gates[np.flatnonzero(gates[:, 5] != 0)[-1], 2])              # an M31 witness: a hint
    adds = np.flatnonzero((gates[:, 3] == 1) & (gates[:, 1] != 0))
    out = int(gates[adds[len(adds) // 2], 2])                              # an add gate's output
    flip = len(ops) // 2
    cases = {}
    for name, var, word, value in (("hint", hint, 0, None), ("gate output", out, 3, None), ("variable 2", 2, 0, None),
                                   ("a word set to P", int(gates[len(gates) // 2, 0]), 1, U.P),
                                   ("witness-op bit", int(ops[flip, 1]), 0, None)):
        t = v.copy()
        t[var, word] = (t[var, word] ^ 1) if value is None else value
        cases[name] = (t, U.model_check(gates, ops, t))
        assert cases[name][1] != NONE, name
    return cases


@pytest.mark.parametrize("layout", ["by_proof", "by_variable"])
def test_circuit_check_names_the_models_row(rsv, ctx, level10, layout):
    v, gates, ops = level10["vars"], level10["gates"], level10["ops"]
    assert U.model_check(gates, ops, v) == NONE
    cases = _tampered(level10)
    names = list(cases)
    ctx.set_option("witness_layout", layout)
    try:
        by_variable = layout == "by_variable"
        for prog in (level10["circ"], level10["wp"]):
            ok, bad = _check(ctx, prog, np.stack([v] + [cases[k][0] for k in names]), by_variable)
            print(layout, {k: (int(bad[1 + i]), cases[k][1]) for i, k in enumerate(names)})
            assert ok.tolist() == [1] + [0] * len(names) and bad.tolist() == [NONE] + [cases[k][1] for k in names]
        # a batch of 70: tampered at 63 and 64, slot 5 masked on entry (and tampered: it is not looked at)
        batch = np.stack([v] * 70)
        batch[63], batch[64], batch[5] = cases["gate output"][0], cases["hint"][0], cases["variable 2"][0]
        ok, bad = _check(ctx, level10["circ"], batch, by_variable, ok=[0 if p == 5 else 1 for p in range(70)])
        want_bad = [cases["gate output"][1] if p == 63 else cases["hint"][1] if p == 64 else NONE for p in range(70)]
        assert ok.tolist() == [0 if p in (5, 63, 64) else 1 for p in range(70)] and bad.tolist() == want_bad
    finally:
        ctx.set_option("witness_layout", "by_proof")


# ---------------------------------------------------------------- 4. the small circuits through the whole chain
def _verify_both(rsv, ctx, proof, cfg, inputs):
    """-> ((accept, reason) of the library, of the C oracle) for one proof."""
    acc, reason = rsv.verify_batch([proof], cfg, inputs)
    oacc, oreason = ob.verify_batch([proof], cfg, inputs)
    return (int(acc[0]), int(reason[0])), (int(oacc[0]), int(oreason[0]))


def _circuit(rsv, b):
    return rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, b.witness_ops)


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "pow%d-blowup%d-last%d-q%d" % (c[0], c[1], c[2], c[3]))
@pytest.mark.parametrize("kind", U.KINDS)
def test_small_circuit_through_the_whole_chain(rsv, ctx, kind, config):
    b = U.build(kind)
    ppre, ptr, qpre, qtr, lp, lq = U.columns(b)
    circ = _circuit(rsv, b)
    assert circ.trace_sizes() == (lp, lq) and (lp + 2 > lq + 3) == (kind == "S2")
    ch, cfg = _run(rsv, ctx, circ, [b], config)
    a = ch.numpy()
    assert a["acc"].tolist() == [1] and a["bad_row"].tolist() == [NONE] and a["bad_flow"].tolist() == [NONE]
    got_pre = circ.preprocessed(b.variables)
    assert np.array_equal(got_pre[0], ppre) and np.array_equal(got_pre[1], qpre)
    assert np.array_equal(a["plonk"][0], ptr) and np.array_equal(a["poseidon"][0], qtr)
    assert a["ops"][0].tolist() == [U.OP_CONSTANT]
    z, alpha = tuple(int(x) for x in a["draws"][0, 0:4]), tuple(int(x) for x in a["draws"][0, 4:8])
    ip, iq, sums, ok = R.interaction(ppre, ptr, qpre, qtr, z, alpha, lp, lq)
    assert ok and np.array_equal(a["int_plonk"][0], ip) and np.array_equal(a["int_poseidon"][0], iq)
    assert a["sums"][0].tolist() == [list(sums[0]), list(sums[1])]
    assert a["ok"].tolist() == [1] and a["low_degree"].tolist() == [1]
    proofs = ch.proofs()
    blob, offsets = ch.pack(exact=True)
    assert offsets.cpu().tolist() == [0, len(proofs[0])] and blob.cpu().numpy().tobytes() == proofs[0]
    assert np.frombuffer(proofs[0][:8], np.uint32).tolist() == [lp, lq]
    mine, oracle = _verify_both(rsv, ctx, proofs[0], cfg, b.inputs)
    print(kind, config, "library", mine, "oracle", oracle, "bytes", len(proofs[0]))
    assert mine == (1, 0) and oracle == (1, 0)
    wrong = b.inputs[:3] + [(4, (12, 0, 0, 0))]                            # another public input: the logup sum is off
    mine, oracle = _verify_both(rsv, ctx, proofs[0], cfg, wrong)
    assert mine[0] == 0 and mine == oracle
    circ.close()


def test_batch_of_three_witnesses_each_with_its_own_input(rsv, ctx):
    """Three witnesses of S1 that differ in the public input, the hints and the witness-op bit: each slot verifies with its
    own inputs and not with a neighbour's."""
    builts = [U.build("S1", pub=(11 + 7 * k, 0, 0, 0), seed=1 + k, bit=k % 2) for k in range(3)]
    assert all(np.array_equal(b.gates[:, [0, 1, 2, 4, 5]], builts[0].gates[:, [0, 1, 2, 4, 5]]) for b in builts)
    circ = _circuit(rsv, builts[0])
    ch, cfg = _run(rsv, ctx, circ, builts, CONFIGS[0])
    a, proofs = ch.numpy(), ch.proofs()
    assert a["acc"].tolist() == [1, 1, 1] and a["ok"].tolist() == [1, 1, 1]
    assert a["ops"][:, 0].tolist() == [U.OP_CONSTANT * (k % 2) for k in range(3)]
    for k, b in enumerate(builts):
        assert np.array_equal(a["plonk"][k], U.columns(b)[1])
        assert _verify_both(rsv, ctx, proofs[k], cfg, b.inputs) == ((1, 0), (1, 0)), k
        mine, oracle = _verify_both(rsv, ctx, proofs[k], cfg, builts[(k + 1) % 3].inputs)
        assert mine[0] == 0 and mine == oracle, k
    circ.close()


# ---------------------------------------------------------------- 5. a wrong witness is data
def test_a_wrong_witness_is_data(rsv, ctx):
    good = [U.build("S1", pub=(11, 0, 0, 0), seed=1), U.build("S1", pub=(18, 0, 0, 0), seed=2)]
    wrong = U.build("S1", pub=(25, 0, 0, 0), seed=3)
    row = int(np.flatnonzero((wrong.gates[:, 3] == 0) & (wrong.gates[:, 4] == 0))[0])   # a multiply gate's output
    wrong.variables[wrong.gates[row, 2], 0] ^= 1
    want_row = U.model_check(wrong.gates, wrong.witness_ops, wrong.variables)
    assert want_row == row
    circ = _circuit(rsv, good[0])
    solo = []
    for b in good:
        ch, cfg = _run(rsv, ctx, circ, [b], CONFIGS[0])
        solo.append(ch.proofs()[0])
    batch = [good[0], wrong, good[1]]
    ch, cfg = _run(rsv, ctx, circ, batch, CONFIGS[0])
    a = ch.numpy()
    assert a["acc"].tolist() == [1, 0, 1] and a["bad_row"].tolist() == [NONE, want_row, NONE] and a["ok"].tolist() == [1, 0, 1]
    assert ch.proofs() == [solo[0], None, solo[1]]
    blob, offsets = ch.pack()
    offsets, blob = offsets.cpu().tolist(), blob.cpu().numpy()
    assert offsets == [0, len(solo[0]), len(solo[0]), len(solo[0]) + len(solo[1])]
    assert blob[:offsets[1]].tobytes() == solo[0] and blob[offsets[2]:offsets[3]].tobytes() == solo[1]
    # unchecked: the chain completes, and both verifiers reject that proof for the same reason
    ch, cfg = _run(rsv, ctx, circ, batch, CONFIGS[0], check=False)
    proofs = ch.proofs()
    assert ch.numpy()["acc"].tolist() == [1, 1, 1] and proofs[0] == solo[0] and proofs[2] == solo[1] and proofs[1] is not None
    mine, oracle = _verify_both(rsv, ctx, proofs[1], cfg, wrong.inputs)
    print("wrong witness, unchecked: library", mine, "oracle", oracle)
    assert oracle[0] == 0 and mine == oracle
    circ.close()
