"""A caller's circuit evaluated on the GPU (`-m gpu`): rsv_circuit_eval_dev through Context.circuit_eval and Chain.evaluate.

1 runs the four circuits of tests/circuit_eval_ref.py at 1, 3 and 70 witnesses (a second workgroup of the per-witness kernels,
lanes 63 and 64 masked) that differ in seed, public input and witness bit, under both layouts and both forced launch forms:
variables, flow and swap are the oracle's, word for word, the chain's 0xffffffff prefill shows that no word of an accepted
witness stays unwritten, and a skipped witness keeps the prefill.  2: input words at or above P.  3: a wrong free input is
data — Chain.evaluate(check=True) names the row or invocation the numpy model of the reference's two checks names on the
evaluated vector.  3b: a swap variable that is no bit, which the evaluation and the check treat differently.  4: evaluate
-> ... -> pack for S1 to S3 under both configurations of tests/test_user_circuit_gpu.py.  5: the level10-1 recursion circuit as a created evaluation program reproduces rsv_witness_eval_dev's vector and flow and the
chain puts out level11-1.bin byte for byte."""
import numpy as np
import pytest

from tests import circuit_eval_ref as E
from tests import oracle_binding as ob
from tests import user_circuit_ref as U
from tests.chain_harness import DEV, FILL, chain, inputs_of, masked_past_64, pin_of, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
SRC, DST = "level10-1.bin", "level11-1.bin"
NONE = U.NONE
CONFIGS = [(3, 1, 0, 9), (8, 2, 2, 16)]   # the two of profiles/HISTORY.md "Caller's circuits"
FORMS = ["per_level", "walk"]
LAYOUTS = ["by_proof", "by_variable"]
_BUILT = {}


@pytest.fixture(scope="module")
def ctx(rsv):
    c = rsv.Context(0)
    yield c
    c.close()


def witness(kind, k):
    """Witness k of a kind: its own seed, public input and bit."""
    if (kind, k) not in _BUILT:
        _BUILT[kind, k] = E.build(kind, pub=(11 + 7 * k, 0, 0, 0), seed=1 + k, bit=k % 2)
    return _BUILT[kind, k]


def _circuit(rsv, b):
    return rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, **E.create_args(b))


def _evaluate(rsv, ctx, circ, inputs, flow_in, layout="by_proof", form="auto", mask=None, check=False, config=CONFIGS[0]):
    """-> (the Chain, variables [n, n_vars, 4], flow, swap) after Chain.evaluate under a layout and a launch form."""
    cfg = rsv.PcsConfig(*config)
    ch = rsv.Chain(ctx, circ, len(inputs), cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, device=DEV)
    ctx.set_option("witness_layout", layout)
    ctx.set_option("circuit_eval_form", form)
    try:
        ch.evaluate(inputs, flow_in, check=check, by_variable=layout == "by_variable", mask=mask)
        ctx.synchronize()
    finally:
        ctx.set_option("witness_layout", "by_proof")
        ctx.set_option("circuit_eval_form", "auto")
    variables = u32(ch._vars)
    return ch, (variables.transpose(1, 0, 2) if layout == "by_variable" else variables), u32(ch._flow), ch._swap.cpu().numpy()


# ---------------------------------------------------------------- 1. the oracle's witnesses, word for word
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("kind", E.KINDS)
def test_evaluates_the_oracles_witnesses(rsv, ctx, kind, n, layout, form):
    builts = [witness(kind, k) for k in range(n)]
    circ = _circuit(rsv, builts[0])
    mask = masked_past_64(n) if n == 70 else None
    inputs, flow_in = np.stack([E.inputs_of(b) for b in builts]), np.stack([E.flow_in_of(b) for b in builts])
    ch, variables, flow, swap = _evaluate(rsv, ctx, circ, inputs, flow_in, layout, form, mask=mask)
    a = ch.numpy()
    assert a["acc"].tolist() == (mask or [1] * n) and a["bad_input"].tolist() == [NONE] * n
    free = np.repeat((builts[0].flow_wires[:, :2] == 0) & (E.links_of(builts[0].cs) == 0), 8, axis=1)
    for k, b in enumerate(builts):
        if mask and not mask[k]:   # untouched: the prefill, and the words the caller gave
            assert (variables[k] == FILL).all() and (swap[k] == 7).all() and (flow[k, :, 16:] == FILL).all()
            assert np.array_equal(flow[k, :, :16], np.where(free, flow_in[k, :, :16], FILL))
            continue
        assert np.array_equal(variables[k], b.variables), (k, np.flatnonzero((variables[k] != b.variables).any(axis=1))[:8])
        assert np.array_equal(flow[k], b.flow), (k, np.flatnonzero((flow[k] != b.flow).any(axis=1))[:8])
        assert np.array_equal(swap[k], b.swap), k
    circ.close()


# ---------------------------------------------------------------- 2. an input word that is no M31
@pytest.mark.parametrize("form", FORMS)
def test_an_input_word_at_p_clears_that_witness_only(rsv, ctx, form):
    builts = [witness("S1", k) for k in range(3)]
    circ = _circuit(rsv, builts[0])
    inputs, flow_in = np.stack([E.inputs_of(b) for b in builts]), np.stack([E.flow_in_of(b) for b in builts])
    n_inputs = inputs.shape[1]
    assert n_inputs >= 4
    one, two = inputs.copy(), inputs.copy()
    one[1, 2, 3] = U.P
    two[2, n_inputs - 1, 0] = U.P
    two[2, 1, 2] = 0xFFFFFFFF
    for bad, want_ok, want_slot in ((one, [1, 0, 1], [NONE, 2, NONE]), (two, [1, 1, 0], [NONE, NONE, 1])):
        ch, variables, flow, swap = _evaluate(rsv, ctx, circ, bad, flow_in, form=form)
        a = ch.numpy()
        assert a["acc"].tolist() == want_ok and a["bad_input"].tolist() == want_slot
        for k, b in enumerate(builts):
            if want_ok[k]:
                assert np.array_equal(variables[k], b.variables) and np.array_equal(flow[k], b.flow) and np.array_equal(swap[k], b.swap)
            else:   # written all the same, with canonical words
                assert (variables[k] < U.P).all() and (flow[k] < U.P).all() and (swap[k] <= 1).all()
    circ.close()


# ---------------------------------------------------------------- 3. a wrong free input is data
def _slot_of(b, variable):
    h = E.hints_of(b.cs)
    return int(h[(h[:, 0] == variable) & (h[:, 1] == E.INPUT)][0, 3])


@pytest.mark.parametrize("kind", ["S1", "S4"])
def test_a_wrong_free_input_is_reported_by_the_checks(rsv, ctx, kind):
    """Witness 0 is sound; 1: the public input is no M31 (its row enforces one); 2: a swap bit that is an input is 2 (S1), or
    the bit-decomposed value does not fit its five bits (S4)."""
    b = witness(kind, 0)
    circ = _circuit(rsv, b)
    inputs, flow_in = np.stack([E.inputs_of(b)] * 3), np.stack([E.flow_in_of(b)] * 3)
    inputs[1, _slot_of(b, 4), 1] = 5
    if kind == "S1":
        addr = int(b.flow_wires[b.flow_wires[:, 4] != 0][0, 4])
        inputs[2, _slot_of(b, addr), 0] = 2
    else:
        src = int(E.hints_of(b.cs)[E.hints_of(b.cs)[:, 1] == E.BIT][0, 2])
        inputs[2, _slot_of(b, src), 0] = 32 + 5
    _, variables, flow, _ = _evaluate(rsv, ctx, circ, inputs, flow_in)
    want_row, want_flow = [], []
    for k in range(3):
        row = U.model_check(b.gates, b.witness_ops, variables[k])
        want_row.append(row)
        want_flow.append(U.model_flow(b.gates, b.flow_wires, variables[k], flow[k])[0] if row == NONE else NONE)   # a failed witness is skipped
    print(kind, "rows", want_row, "invocations", want_flow)
    assert want_row[0] == NONE and want_flow[0] == NONE and want_row[1] != NONE and (want_row[2] != NONE or want_flow[2] != NONE)
    ch, _, _, _ = _evaluate(rsv, ctx, circ, inputs, flow_in, check=True)
    a = ch.numpy()
    assert a["bad_input"].tolist() == [NONE] * 3 and a["bad_row"].tolist() == want_row and a["bad_flow"].tolist() == want_flow
    assert a["acc"].tolist() == [1, 0, 0]
    circ.close()


# ---------------------------------------------------------------- 3b. a swap variable that is no bit
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_swap_variable_that_is_no_bit(rsv, ctx, layout, form):
    """The one thing the evaluation and the check do differently with the same invocation.  S1's swapped invocation; witness
    0: the swap variable is 2, witness 1: it is 1 + 5 i, witness 2: untouched.  rsv_circuit_eval_dev takes the low bit of
    the first coordinate, permutes, and keeps ok; rsv_circuit_flow_dev on the variables it wrote asks for the QM31 0 or 1:
    it names the invocation, writes the record of a zero state and clears ok, for the first two witnesses only."""
    import torch
    b = witness("S1", 0)
    circ = _circuit(rsv, b)
    at = int(np.flatnonzero(b.flow_wires[:, 4])[0])
    slot = _slot_of(b, int(b.flow_wires[at, 4]))
    inputs, flow_in = np.stack([E.inputs_of(b)] * 3), np.stack([E.flow_in_of(b)] * 3)
    inputs[0, slot] = (2, 0, 0, 0)
    inputs[1, slot] = (1, 5, 0, 0)
    ch, variables, flow, swap = _evaluate(rsv, ctx, circ, inputs, flow_in, layout, form)
    a = ch.numpy()
    assert a["acc"].tolist() == [1, 1, 1] and a["bad_input"].tolist() == [NONE] * 3
    tables = (b.gates, b.flow_wires, E.links_of(b.cs), b.n_vars)
    exported = circ.eval_export()
    for k in range(3):
        want_vars, want_flow, want_swap = E.model_eval(*exported, tables, inputs[k], flow_in[k])
        assert np.array_equal(variables[k], want_vars) and np.array_equal(flow[k], want_flow) and np.array_equal(swap[k], want_swap), k
    assert swap[:, at].tolist() == [0, 1, 1]
    assert np.array_equal(variables[2], b.variables) and np.array_equal(flow[2], b.flow)
    # the check, on the same variables and the flow the evaluation left
    want = [U.model_flow(b.gates, b.flow_wires, variables[k], flow[k]) for k in range(3)]
    assert [w[0] for w in want] == [at, at, NONE]
    zero_out = U.permute([0] * 16)
    assert want[0][1][at, 16:].tolist() == zero_out and want[1][1][at, 16:].tolist() == zero_out
    d_flow, d_swap = ch._flow.clone(), torch.full_like(ch._swap, 7)
    ok, bad = torch.ones(3, dtype=torch.uint8, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV)
    ctx.set_option("witness_layout", layout)
    try:
        ctx.circuit_flow(circ, ch._vars, 3, d_flow, d_swap, ok, bad)
        ctx.synchronize()
    finally:
        ctx.set_option("witness_layout", "by_proof")
    assert u32(bad).tolist() == [at, at, NONE] and ok.cpu().tolist() == [0, 0, 1]
    got_flow, got_swap = u32(d_flow), d_swap.cpu().numpy()
    for k in range(3):
        assert np.array_equal(got_flow[k], want[k][1]) and np.array_equal(got_swap[k], want[k][2]), k
    circ.close()


# ---------------------------------------------------------------- 4. from the inputs to the packed proof
def _finish(ch, cfg):
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch, stage)()
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.open()
    ch.fri_open()
    return ch


def _verify_both(rsv, proof, cfg, inputs):
    acc, reason = rsv.verify_batch([proof], cfg, inputs)
    oacc, oreason = ob.verify_batch([proof], cfg, inputs)
    return (int(acc[0]), int(reason[0])), (int(oacc[0]), int(oreason[0]))


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "pow%d-blowup%d-last%d-q%d" % (c[0], c[1], c[2], c[3]))
@pytest.mark.parametrize("kind", U.KINDS)
def test_evaluate_through_the_whole_chain(rsv, ctx, kind, config):
    b = witness(kind, 0)
    circ = _circuit(rsv, b)
    cfg = rsv.PcsConfig(*config)
    ch, variables, flow, _ = _evaluate(rsv, ctx, circ, E.inputs_of(b)[None], E.flow_in_of(b)[None], check=True, config=config)
    assert np.array_equal(variables[0], b.variables) and np.array_equal(flow[0], b.flow)
    _finish(ch, cfg)
    a = ch.numpy()
    assert a["acc"].tolist() == [1] and a["bad_row"].tolist() == [NONE] and a["bad_flow"].tolist() == [NONE] and a["ok"].tolist() == [1]
    assert np.array_equal(a["plonk"][0], U.columns(b)[1])
    proofs = ch.proofs()
    blob, offsets = ch.pack(exact=True)
    assert offsets.cpu().tolist() == [0, len(proofs[0])] and blob.cpu().numpy().tobytes() == proofs[0]
    assert _verify_both(rsv, proofs[0], cfg, b.inputs) == ((1, 0), (1, 0))
    wrong = b.inputs[:3] + [(4, (12, 0, 0, 0))]
    mine, oracle = _verify_both(rsv, proofs[0], cfg, wrong)
    assert mine[0] == 0 and mine == oracle
    circ.close()


# ---------------------------------------------------------------- 5. the real size, once
W_COPY, W_BIT, W_FLOW, W_CINV = 4, 10, 11, 8


def test_level10_as_a_created_evaluation_program(rsv, ctx):
    """The recursion circuit's own program turned into hints: the arithmetic hint ops go to their kinds, reads of a
    permutation's output are left to rule 3, everything that reads the proof (and a read of a permutation's input word)
    becomes an INPUT whose value is rsv_witness_eval_dev's own."""
    wp = program_of(rsv, pin_of(SRC))
    built = chain(rsv, ctx, wp, [read_proof(SRC)], inputs_of(SRC), 1, upto="witness")
    ctx.synchronize()
    assert built.acc.cpu().tolist() == [1]
    variables, flow, swap = u32(built._vars)[0].copy(), u32(built._flow)[0].copy(), built._swap.cpu().numpy()[0].copy()
    gates, ops = wp.gates()
    prog = wp.export()
    wires = np.ascontiguousarray(prog.flow_wires, dtype=np.uint32)
    hints, inputs = [], []
    for op, dst, a, _b, i0, i1, _i2, _i3 in np.asarray(prog.instr).tolist():
        if op < W_COPY:
            continue                                                  # constants and gates: rules 1 and 4
        if op <= W_BIT:
            hints.append((dst, op - W_COPY + E.COPY, a, i0 if op >= W_CINV else 0))
            continue
        if op == W_FLOW and (i1 >> 2) >= 4:
            continue                                                  # an output word: rule 3
        hints.append((dst, E.INPUT, 0, len(inputs)))
        inputs.append(variables[dst])
    wp.close()
    circ = rsv.Circuit(gates, wires, len(variables), 3, ops, hints=np.array(hints, np.uint32), n_inputs=len(inputs))
    n_inputs, n_levels, n_instr = circ.eval_info()
    flow_in = flow.copy()
    flow_in[:, 16:] = 0
    for h in range(2):
        flow_in[wires[:, h] != 0, 8 * h:8 * h + 8] = 0
    print("level10: inputs", n_inputs, "levels", n_levels, "instructions", n_instr, "invocations", len(wires), "free halves", int((wires[:, :2] == 0).sum()))
    want, cfg = read_proof(DST), fixture_cfg(DST)
    config = (cfg.pow_bits, cfg.log_blowup_factor, cfg.log_last_layer_degree_bound, cfg.n_queries)
    for form in FORMS:
        ch, got, got_flow, got_swap = _evaluate(rsv, ctx, circ, np.array(inputs, np.uint32)[None], flow_in[None], form=form, check=form == "walk", config=config)
        assert np.array_equal(got[0], variables), (form, np.flatnonzero((got[0] != variables).any(axis=1))[:8])
        assert np.array_equal(got_flow[0], flow) and np.array_equal(got_swap[0], swap), form
    _finish(ch, cfg)
    a = ch.numpy()
    assert a["acc"].tolist() == [1] and a["bad_row"].tolist() == [NONE] and a["bad_flow"].tolist() == [NONE] and a["ok"].tolist() == [1]
    assert ch.proofs()[0] == want
    blob, offsets = ch.pack(exact=True)
    assert offsets.cpu().tolist() == [0, len(want)] and blob.cpu().numpy().tobytes() == want
    circ.close()
