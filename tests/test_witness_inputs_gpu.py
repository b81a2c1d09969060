"""Recursing over a batch in which every proof has its own public inputs (`-m gpu`): rsv_witness_program_build_inputs,
rsv_witness_eval_inputs_dev, rsv_witness_eval_groups_inputs_dev, Chain.witness(d_inputs=...).  Everything is exact on
32-bit words and verdict bytes.

The inner proofs are the smallest the project proves: circuit S1 of tests/user_circuit_ref.py under CONFIG, witness i with
the public input (11 + i, 0, 0, 0), evaluated and proved by the chain itself; their statements are the chain's own
(Chain.inputs(): the records (1, one), (2, i), (3, j), (4, pub)).  One program, built from proof 0 with the first three
records fixed and the fourth the proof's own, then serves every proof: variable 4 of row i is 11 + i."""
import numpy as np
import pytest

from tests import circuit_eval_ref as E
from tests import oracle_binding as ob
from tests import witness_inputs_ref as W
from tests.chain_harness import DEV, FILL, LAUNCH_FORMS_FEW as FORMS, launch_form, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = W.P
R_PARSE, R_LOGUP, R_DUP_QUERY = 1, 3, 5
E_NULL, E_SIZE = -1, -2
CONFIG = (3, 1, 0, 9)          # (pow_bits, log_blowup, log_last, n_queries): the smallest the project proves
N = 70                         # past one 64-lane workgroup: the wide form, a partly filled workgroup
ONE = (1, 0, 0, 0)


@pytest.fixture(scope="module")
def ctx(rsv):
    c = rsv.Context(0)
    yield c
    c.close()


def _finish(ch, cfg):
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch, stage)()
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.open()
    ch.fri_open()
    return ch


def _dev(a, dtype=np.uint32):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).to(DEV)


def _full(shape, flag=False):
    import torch
    return torch.full(shape, 0xFF if flag else -1, dtype=torch.uint8 if flag else torch.int32, device=DEV)


class Inner:
    pass


@pytest.fixture(scope="module")
def inner(rsv, ctx):
    """N proofs of S1 with statements 11 + i, their packed pair on the device, their statements, and the program.
    Nine queries into 2^11 positions: about one proof in sixty draws a position twice, which the verifier rejects as the
    reference does (RSV_R_DUP_QUERY).  Such a witness is made again from another seed, so that all N proofs verify."""
    import torch
    s = Inner()
    s.cfg = rsv.PcsConfig(*CONFIG)
    seeds = [1 + i for i in range(N)]
    circ = None
    for _ in range(4):
        s.builts = [E.build("S1", pub=(11 + i, 0, 0, 0), seed=seeds[i], bit=i % 2) for i in range(N)]
        b0 = s.builts[0]
        if circ is None:
            circ = rsv.Circuit(b0.gates, b0.flow_wires, b0.n_vars, b0.num_input, **E.create_args(b0))
        ch = rsv.Chain(ctx, circ, N, s.cfg.log_blowup_factor, log_last=s.cfg.log_last_layer_degree_bound, fill=FILL, caps=True, device=DEV)
        ch.evaluate(np.stack([E.inputs_of(b) for b in s.builts]), np.stack([E.flow_in_of(b) for b in s.builts]), check=True)
        _finish(ch, s.cfg)
        a = ch.numpy()
        assert a["acc"].tolist() == [1] * N and a["ok"].tolist() == [1] * N
        acc, reason = ch.verify(s.cfg)
        ctx.synchronize()
        acc, reason = acc.cpu().tolist(), reason.cpu().tolist()
        assert all(r in (0, R_DUP_QUERY) for r in reason), reason
        if all(acc):
            break
        seeds = [sd if ok else sd + 1000 for sd, ok in zip(seeds, acc)]
    assert all(acc), (acc, reason)
    s.statements = ch.inputs().clone()                       # int32[N, 4, 5]
    assert u32(s.statements)[:, 3].tolist() == [[4, 11 + i, 0, 0, 0] for i in range(N)]
    s.own = s.statements[:, 3:, :].contiguous()              # minus the fixed records: int32[N, 1, 5]
    s.proofs = ch.proofs()
    s.d_blob, s.d_offsets = ch.pack()
    s.inputs = [b.inputs for b in s.builts]
    s.fixed = s.inputs[0][:3]
    assert s.fixed == [(1, ONE), (2, (0, 1, 0, 0)), (3, (0, 0, 1, 0))]
    s.wp = rsv.WitnessProgram.build(s.proofs[0], s.cfg, s.inputs[0], n_fixed=3)
    s.circ = circ
    torch.cuda.synchronize()
    yield s
    s.wp.close()
    circ.close()


_ORACLE = {}


def _oracle_variables(inner, i):
    """The oracle's `variables` of the circuit that verifies proof i with its input allocated PUBLIC."""
    if i not in _ORACLE:
        c, _ = W.build_circuit(inner.proofs[i], inner.inputs[i], 3)
        assert c.num_input == 4
        _ORACLE[i] = np.array(c.variables, dtype=np.uint32)
    return _ORACLE[i]


def _upload(rsv, proofs):
    import torch
    blob, offsets = rsv.pack(proofs)
    return torch.from_numpy(blob.copy()).to(DEV), torch.from_numpy(offsets.astype(np.int64)).to(DEV)


def _eval(rsv, ctx, wp, pair, n, fixed, d_own, layout="by_proof", form=(0, 0, 0)):
    """Context.witness with d_inputs under a layout and a launch form, outputs prefilled -> (variables [n, n_vars, 4], flow,
    swap, accept, reason)."""
    F = wp.shape.flow_count
    by_variable = layout == "by_variable"
    d_vars = _full((wp.n_vars, n, 4) if by_variable else (n, wp.n_vars, 4))
    d_flow, d_swap, d_acc, d_reason = _full((n, F, 32)), _full((n, F), True), _full((n,), True), _full((n,), True)
    ctx.set_option("witness_layout", layout)
    try:
        with launch_form(ctx, form, n):
            ctx.witness(wp, *pair, n, d_vars, d_acc, d_reason, inputs=fixed, d_flow=d_flow, d_flow_swap=d_swap, d_inputs=d_own)
            ctx.synchronize()
    finally:
        ctx.set_option("witness_layout", "by_proof")
    v = u32(d_vars)
    return (v.transpose(1, 0, 2) if by_variable else v), u32(d_flow), d_swap.cpu().numpy(), d_acc.cpu().numpy(), d_reason.cpu().numpy()


# ---------------------------------------------------------------- 1. the witness vectors
def test_the_program_knows_its_inputs(rsv, inner):
    wp = inner.wp
    n_fixed, n_own, idx = wp.inputs()
    assert (n_fixed, n_own, idx.tolist()) == (3, 1, [4]) and wp.num_input == 4
    rows, _ = wp.gates()
    assert rows[4].tolist() == [4, 0, 4, 1, 0, 1]
    prog = wp.export()
    at = np.flatnonzero(prog.instr[:, 0] == W.W_INPUT)
    assert prog.instr[at].tolist() == [[W.W_INPUT, 4, 0, 0, 0, 0, 0, 0]] and at[0] < prog.level_offsets[1]
    # the program has the narrow tail the strip form is launched for (at least 8 last levels of at most 32 instructions,
    # csrc/witness_api.inc) behind wider levels, so the forced forms below do run k_witness_strip<WitnessInputArgs> and the level kernels
    widths = np.diff(prog.level_offsets.astype(np.int64))
    tail = len(widths) - (np.flatnonzero(widths > 32)[-1] + 1)
    assert 8 <= tail < len(widths) and widths[0] > 1536
    old = rsv.WitnessProgram.build(inner.proofs[0], inner.cfg, inner.inputs[0])
    assert old.inputs()[:2] == (4, 0) and old.num_input == 3 and old.n_vars == wp.n_vars + 9
    old.close()


@pytest.mark.parametrize("layout", ["by_proof", "by_variable"])
@pytest.mark.parametrize("n", [1, 3, N])
def test_rows_are_the_oracles_variables(rsv, ctx, inner, n, layout):
    """n = 1, 3 and 70 proofs with their own statements: every proof accepted, variable 4 of row i is 11 + i; the rows of
    the first three are the oracle's, word for word; the flow is the per-proof verifying call's."""
    pair = _upload(rsv, inner.proofs[:n])
    variables, flow, swap, acc, reason = _eval(rsv, ctx, inner.wp, pair, n, inner.fixed, inner.own[:n].contiguous(), layout)
    assert acc.tolist() == [1] * n and reason.tolist() == [0] * n, reason.tolist()
    assert variables[:, 4].tolist() == [[11 + i, 0, 0, 0] for i in range(n)]
    for i in range(min(n, 3)):
        want = _oracle_variables(inner, i)
        assert variables[i].shape == want.shape and np.array_equal(variables[i], want), i
    F = inner.wp.shape.flow_count
    d_acc, d_reason = _full((n,), True), _full((n,), True)
    d_flow, d_swap, d_count = _full((n, F, 32)), _full((n, F), True), _full((n,))
    ctx.verify_hints(*pair, n, d_acc, d_reason, cfg=inner.cfg, inputs=inner.fixed, d_flow=d_flow, d_flow_swap=d_swap, d_flow_count=d_count,
                     d_inputs=inner.statements[:n].contiguous(), n_inputs=4)
    ctx.synchronize()
    assert d_acc.cpu().tolist() == [1] * n and u32(d_count).tolist() == [F] * n
    assert np.array_equal(flow, u32(d_flow)) and np.array_equal(swap, d_swap.cpu().numpy())


@pytest.mark.parametrize("layout", ["by_proof", "by_variable"])
@pytest.mark.parametrize("n", [3, N])
def test_every_launch_form_reads_the_inputs(rsv, ctx, inner, n, layout):
    """By the default rule batches this small run the whole program in one launch (k_witness_small<WitnessInputArgs>), so the other
    instantiations over WitnessInputArgs are forced through the options, as the constant form's tests force theirs: the
    level-per-launch form — below 64 proofs k_witness_level<WitnessInputArgs>, from 64 on k_witness_level_wide<WitnessInputArgs>
    with a partly filled second block, level 0 with its W_INPUT among them — with the tail as a strip
    (k_witness_strip<WitnessInputArgs>) and in one launch.
    One proof is given a neighbour's statement, so that a rejected row sits among the accepted ones.  Under every form: the
    verdicts, variable 4, every byte of the default form's outputs for the accepted proofs, and the oracle's rows."""
    pair = _upload(rsv, inner.proofs[:n])
    bad = 1 if n == 3 else 63
    rec = u32(inner.own[:n]).copy()
    rec[bad, 0, 1] = rec[bad - 1, 0, 1]
    d_own = _dev(rec)
    good = np.arange(n) != bad
    want = _eval(rsv, ctx, inner.wp, pair, n, inner.fixed, d_own, layout)
    assert want[3].tolist() == good.astype(int).tolist() and want[4][bad] == R_LOGUP
    assert want[0][good, 4, 0].tolist() == [11 + i for i in range(n) if i != bad]
    for i in (0, 2):
        assert np.array_equal(want[0][i], _oracle_variables(inner, i))
    for form in FORMS[:-1]:
        got = _eval(rsv, ctx, inner.wp, pair, n, inner.fixed, d_own, layout, form)
        assert got[3].tolist() == want[3].tolist() and got[4].tolist() == want[4].tolist(), form
        for a, b in zip(want[:3], got[:3]):
            assert np.array_equal(a[good], b[good]), form


def test_the_device_pair_of_the_inner_chain_is_taken_as_it_is(rsv, ctx, inner):
    """The packed pair Chain.pack() left (slots sized by the capacities) and the statements Chain.inputs() left: all 70."""
    variables, _, _, acc, _ = _eval(rsv, ctx, inner.wp, (inner.d_blob, inner.d_offsets), N, inner.fixed, inner.own)
    assert acc.tolist() == [1] * N and variables[:, 4, 0].tolist() == [11 + i for i in range(N)]
    assert np.array_equal(variables[2], _oracle_variables(inner, 2))


# ---------------------------------------------------------------- 2. equal to the constant form where both exist
def test_without_own_inputs_the_call_is_the_constant_forms(rsv, ctx):
    """n_own = 0 on small_proof.bin x 3 (one of them tampered): variables, flow, swap, accept and reason are
    rsv_witness_eval_dev's bytes, in both layouts."""
    import torch
    small, cfg, shared = read_proof("small_proof.bin"), fixture_cfg("small_proof.bin"), [(1, ONE)]
    wp = rsv.WitnessProgram.build(small, cfg, shared)
    pair = _upload(rsv, [small, ob.tamper(small, 3), small])
    none = torch.zeros((3, 0, 5), dtype=torch.int32, device=DEV)
    try:
        assert wp.inputs()[:2] == (1, 0)
        for layout in ("by_proof", "by_variable"):
            want = _eval(rsv, ctx, wp, pair, 3, shared, None, layout)
            got = _eval(rsv, ctx, wp, pair, 3, shared, none, layout)
            assert want[3].tolist() == [1, 0, 1]
            for a, b in zip(want, got):
                assert a.tobytes() == b.tobytes()
    finally:
        wp.close()


def test_rows_equal_the_constant_programs_through_the_variable_map(rsv, ctx, inner):
    """Proof i under the program built by the constant builder for proof i ALONE (its statement a constant) against row i
    of the one program with own inputs.  The constant circuit allocates the statement as a QM31 constant where the other
    has its public input: ten variables (the value, four M31 constants, five of the recombination) and ten rows instead
    of one of each, at the same place, directly behind the four fixed constants.  So old variable 4 is new variable 4, old 5 .. 13
    have no counterpart, old k is new k - 9; the map is checked on the two gate lists (every row behind the statement's
    is the same row through the map), then on the values."""
    new_rows, _ = inner.wp.gates()
    pair = _upload(rsv, inner.proofs[:3])
    new_vars = _eval(rsv, ctx, inner.wp, pair, 3, inner.fixed, inner.own[:3].contiguous())[0]
    for i in range(3):
        old = rsv.WitnessProgram.build(inner.proofs[i], inner.cfg, inner.inputs[i])
        try:
            assert old.n_vars == inner.wp.n_vars + 9
            to_new = np.concatenate([np.arange(5), np.full(9, -1), np.arange(5, inner.wp.n_vars)]).astype(np.int64)
            old_rows, _ = old.gates()
            assert len(old_rows) == len(new_rows) + 9
            tail = old_rows[14:].astype(np.int64)
            mapped = np.stack([to_new[tail[:, 0]], to_new[tail[:, 1]], to_new[tail[:, 2]], tail[:, 3], np.where(tail[:, 4] != 0, to_new[tail[:, 4]], 0),
                               tail[:, 5]], axis=1)
            assert (mapped[:, :3] >= 0).all()
            ops = inner.wp.gates()[1]
            same = np.ones(len(mapped), bool)
            same[ops[:, 0] - 5] = False                      # rows whose op follows the witness: the templates differ
            assert np.array_equal(mapped[same], new_rows[5:].astype(np.int64)[same])
            assert np.array_equal(np.delete(mapped, 3, axis=1), np.delete(new_rows[5:].astype(np.int64), 3, axis=1))
            one = _upload(rsv, [inner.proofs[i]])
            old_vars = _eval(rsv, ctx, old, one, 1, inner.inputs[i], None)[0][0]
            keep = to_new >= 0
            assert old_vars[4].tolist() == [11 + i, 0, 0, 0]
            assert np.array_equal(old_vars[keep], new_vars[i][to_new[keep]]), i
        finally:
            old.close()


# ---------------------------------------------------------------- 3. rejections
def test_rotated_statements_are_rejected_as_the_oracle_rejects_them(rsv, ctx, inner):
    n = 3
    pair = _upload(rsv, inner.proofs[:n])
    rotated = inner.own[:n].roll(-1, 0).contiguous()
    _, _, _, acc, reason = _eval(rsv, ctx, inner.wp, pair, n, inner.fixed, rotated)
    want = [ob.verify_batch([inner.proofs[i]], inner.cfg, inner.fixed + [(4, (11 + (i + 1) % n, 0, 0, 0))]) for i in range(n)]
    assert [(int(a[0]), int(r[0])) for a, r in want] == [(0, R_LOGUP)] * n
    assert acc.tolist() == [0] * n and reason.tolist() == [R_LOGUP] * n


def test_a_statement_the_circuit_cannot_hold_is_a_parse_error(rsv, ctx, inner):
    """Seven proofs; proof 1's record has another idx, proof 3's value a word 1, proof 5's value word 0 = P: each RSV_R_PARSE,
    the neighbours accepted with the rows they have in the clean batch."""
    n = 7
    pair = _upload(rsv, inner.proofs[:n])
    clean = _eval(rsv, ctx, inner.wp, pair, n, inner.fixed, inner.own[:n].contiguous())
    assert clean[3].tolist() == [1] * n
    rec = u32(inner.own[:n]).copy()
    rec[1, 0, 0] = 5
    rec[3, 0, 2] = 1
    rec[5, 0, 1] = P
    got = _eval(rsv, ctx, inner.wp, pair, n, inner.fixed, _dev(rec))
    assert got[3].tolist() == [1, 0, 1, 0, 1, 0, 1] and got[4].tolist() == [0, R_PARSE, 0, R_PARSE, 0, R_PARSE, 0]
    for i in (0, 2, 4, 6):
        assert np.array_equal(got[0][i], clean[0][i]) and np.array_equal(got[1][i], clean[1][i]) and np.array_equal(got[2][i], clean[2][i])


def test_refusals_come_before_any_device_work(rsv, ctx, inner):
    """RSV_E_NULL / RSV_E_SIZE, and not one output byte changes."""
    import torch
    lib, wp, n = rsv.lib, inner.wp, 3
    F = wp.shape.flow_count
    pair = _upload(rsv, inner.proofs[:n])
    d_own = inner.own[:n].contiguous()
    outs = [_full((n, wp.n_vars, 4)), _full((n, F, 32)), _full((n, F), True), _full((n,), True), _full((n,), True)]
    pc = ctx.prepare_cfg(wp.cfg(), n)
    fixed = rsv.make_inputs(inner.fixed)
    other_idx = rsv.make_inputs([(1, ONE), (2, (0, 1, 0, 0)), (7, (0, 0, 1, 0))])
    raw = torch.zeros(64, dtype=torch.uint8, device=DEV)

    def call(n_=n, fixed_=fixed, n_fixed=3, d_pi=d_own.data_ptr(), n_own=1, d_vars=outs[0].data_ptr(), d_acc=outs[3].data_ptr(), prog=wp._h):
        ctx.acquire_from_torch()
        return lib.rsv_witness_eval_inputs_dev(ctx._h, prog, pair[0].data_ptr(), pair[1].data_ptr(), n_, pc.ref(), fixed_, n_fixed, d_pi, n_own,
                                               d_vars, outs[1].data_ptr(), outs[2].data_ptr(), d_acc, outs[4].data_ptr())
    assert call(d_vars=None) == E_NULL and call(d_acc=None) == E_NULL and call(d_pi=None) == E_NULL and call(fixed_=None) == E_NULL
    assert call(prog=None) == E_NULL
    assert call(n_fixed=2) == E_SIZE and call(n_own=2) == E_SIZE and call(n_own=0) == E_SIZE
    assert call(fixed_=other_idx) == E_SIZE
    assert call(d_pi=raw.data_ptr() + 2) == E_SIZE
    assert call(n_=(1 << 30) // 4 + 1) == E_SIZE                                  # (beyond 2^20 proofs as well: isolated below)
    # what the verifying pass would refuse is refused ahead of the statement kernel too: another configuration, a blob
    # that is not word aligned
    other = ctx.prepare_cfg(rsv.PcsConfig(CONFIG[0], CONFIG[1], CONFIG[2], CONFIG[3] + 1), n)
    ctx.acquire_from_torch()
    assert lib.rsv_witness_eval_inputs_dev(ctx._h, wp._h, pair[0].data_ptr(), pair[1].data_ptr(), n, other.ref(), fixed, 3, d_own.data_ptr(), 1,
                                           outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr()) == E_SIZE
    assert lib.rsv_witness_eval_inputs_dev(ctx._h, wp._h, pair[0].data_ptr() + 2, pair[1].data_ptr(), n, pc.ref(), fixed, 3, d_own.data_ptr(), 1,
                                           outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr()) == E_SIZE
    assert lib.rsv_witness_eval_inputs_dev(ctx._h, wp._h, None, pair[1].data_ptr(), n, pc.ref(), fixed, 3, d_own.data_ptr(), 1,
                                           outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr()) == E_NULL
    # the Python layer refuses a tensor the library would misread: a slice that is not contiguous, too few rows, another type
    for wrong in (inner.statements[:n, 3:, :], inner.own[:n - 1].contiguous(), inner.own[:n].contiguous().to(torch.int64)):
        with pytest.raises(ValueError):
            ctx.witness(wp, *pair, n, outs[0], outs[3], outs[4], inputs=inner.fixed, d_inputs=wrong)
    # the constant forms refuse a program with own inputs
    with pytest.raises(rsv.RsvError) as e:
        ctx.witness(wp, *pair, n, outs[0], outs[3], outs[4], inputs=inner.inputs[0])
    assert e.value.code == E_SIZE
    ctx.synchronize()
    for t in outs:
        assert bool((t == (0xFF if t.dtype == torch.uint8 else -1)).all())
    assert call() == 0                                                            # and the same arguments, unchanged, are taken
    ctx.synchronize()
    assert outs[3].cpu().tolist() == [1] * n


def test_a_created_program_is_checked_against_the_batchs_n_own(rsv, ctx, inner):
    """A program made from instructions has no n_own on record: W_INPUT's imm0 must lie below the call's n_own (RSV_E_SIZE
    otherwise, before any launch); with it the exported program evaluates as the built one does."""
    import torch
    n = 3
    exported = inner.wp.export()
    made = rsv.WitnessProgram(exported)
    pair = _upload(rsv, inner.proofs[:n])
    try:
        with pytest.raises(rsv.RsvError):
            made.inputs()
        with pytest.raises(rsv.RsvError) as e:
            _eval(rsv, ctx, made, pair, n, inner.inputs[0], torch.zeros((n, 0, 5), dtype=torch.int32, device=DEV))
        assert e.value.code == E_SIZE
        got = _eval(rsv, ctx, made, pair, n, inner.fixed, inner.own[:n].contiguous())
        want = _eval(rsv, ctx, inner.wp, pair, n, inner.fixed, inner.own[:n].contiguous())
        for a, b in zip(want, got):
            assert a.tobytes() == b.tobytes()
        # RSV_MAX_INPUT_RECORDS alone: a made program has no n_fixed on record, so 2^20 proofs (allowed) with 1 024 + 1 records
        # each (allowed) are refused for their product only, 2^20 * 1 025 > 2^30, before anything is read
        many = rsv.make_inputs([(k + 10, ONE) for k in range(1024)])
        pc = ctx.prepare_cfg(made.cfg(), n)
        one = inner.own[:1].contiguous()
        ctx.acquire_from_torch()
        assert rsv.lib.rsv_witness_eval_inputs_dev(ctx._h, made._h, pair[0].data_ptr(), pair[1].data_ptr(), 1 << 20, pc.ref(), many, 1024,
                                                   one.data_ptr(), 1, one.data_ptr(), None, None, one.data_ptr(), None) == E_SIZE
        bad = exported.instr.copy()
        bad[np.flatnonzero(bad[:, 0] == W.W_INPUT)[0], 4] = W.MAX_OWN_INPUTS
        exported.instr = bad
        with pytest.raises(rsv.RsvError) as e:
            rsv.WitnessProgram(exported)
        assert e.value.code == -5                                                 # RSV_E_RANGE
    finally:
        made.close()


# ---------------------------------------------------------------- 4. the loop closes
def test_the_loop_closes(rsv, ctx, inner):
    """Chain.witness with the inner chain's packed pair and statements -> ... -> pack(): the outer statements carry the
    inner ones, one verifying call accepts the three outer proofs, the C oracle accepts each under its own statement and
    rejects it under a neighbour's; the reference's two checks pass on the outer witnesses."""
    import torch
    n, wp, cfg = 3, inner.wp, inner.cfg
    och = rsv.Chain(ctx, wp, n, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, device=DEV)
    och.witness((inner.d_blob, inner.d_offsets[:n + 1].contiguous()), inner.fixed, d_inputs=inner.own[:n].contiguous())
    ctx.synchronize()
    assert och.acc.cpu().tolist() == [1] * n
    statements = u32(och.inputs())
    assert statements.shape == (n, 4, 5)
    assert statements.tolist() == [[[1, 1, 0, 0, 0], [2, 0, 1, 0, 0], [3, 0, 0, 1, 0], [4, 11 + i, 0, 0, 0]] for i in range(n)]
    ok, bad_row, bad_flow = torch.ones(n, dtype=torch.uint8, device=DEV), _full((n,)), _full((n,))
    flow, swap = och._flow.clone(), och._swap.clone()
    ctx.circuit_check(wp, och._vars, n, ok, bad_row)
    ctx.circuit_flow(wp, och._vars, n, flow, swap, ok, bad_flow)
    ctx.synchronize()
    assert ok.cpu().tolist() == [1] * n and u32(bad_row).tolist() == [0xFFFFFFFF] * n and u32(bad_flow).tolist() == [0xFFFFFFFF] * n
    assert torch.equal(flow, och._flow) and torch.equal(swap, och._swap)
    _finish(och, cfg)
    acc, reason = och.verify(cfg)
    ctx.synchronize()
    assert acc.cpu().tolist() == [1] * n and reason.cpu().tolist() == [0] * n
    outer = och.proofs()
    for i in range(n):
        own = inner.fixed + [(4, (11 + i, 0, 0, 0))]
        neighbour = inner.fixed + [(4, (11 + (i + 1) % n, 0, 0, 0))]
        assert [int(x[0]) for x in ob.verify_batch([outer[i]], cfg, own)] == [1, 0]
        assert int(ob.verify_batch([outer[i]], cfg, neighbour)[0][0]) == 0


# ---------------------------------------------------------------- 5. groups
def _eval_groups(rsv, ctx, wp, pair, n_groups, fixed, d_own):
    m, F = wp.shape.copies, wp.shape.flow_count
    d_vars, d_acc = _full((n_groups, wp.n_vars, 4)), _full((n_groups,), True)
    d_macc, d_mreason = _full((n_groups * m,), True), _full((n_groups * m,), True)
    d_flow, d_swap = _full((n_groups, m, F, 32)), _full((n_groups, m, F), True)
    ctx.witness_groups(wp, *pair, n_groups, d_vars, d_acc, d_macc, d_mreason, inputs=fixed, d_flow=d_flow, d_flow_swap=d_swap, d_inputs=d_own)
    ctx.synchronize()
    return u32(d_vars), d_acc.cpu().numpy(), d_macc.cpu().numpy().reshape(n_groups, m), d_mreason.cpu().numpy().reshape(n_groups, m)


@pytest.mark.parametrize("n_groups", [3, N])
def test_every_launch_form_of_the_groups_reads_the_inputs(rsv, ctx, inner, n_groups):
    """The grouped instantiations over WitnessGroupInputArgs under the same forms: 3 groups (k_witness_level<A>) and 70
    (k_witness_level_wide<A>, a partly filled second block), group g = proofs 2g and 2g + 1 of the 70, taken round again.
    One member has a neighbour's statement.  Under every form: the verdicts, variables 4 and 5 of every accepted group, the
    default form's rows, and for two groups the oracle's two-member circuit."""
    members = [(2 * g + c) % N for g in range(n_groups) for c in range(2)]
    wp2 = rsv.WitnessProgram.build(inner.proofs[0], inner.cfg, inner.inputs[0], copies=2, n_fixed=3)
    try:
        pair = _upload(rsv, [inner.proofs[m] for m in members])
        rec = u32(inner.own)[members].copy()
        bad_group = 1 if n_groups == 3 else 64
        rec[2 * bad_group + 1, 0, 1] += 1
        d_own = _dev(rec)
        good = np.arange(n_groups) != bad_group
        want = _eval_groups(rsv, ctx, wp2, pair, n_groups, inner.fixed, d_own)
        assert want[1].tolist() == good.astype(int).tolist()
        assert want[2][bad_group].tolist() == [1, 0] and want[3][bad_group].tolist() == [0, R_LOGUP] and want[2][good].all()
        assert want[0][good][:, 4:6, 0].tolist() == [[11 + members[2 * g], 11 + members[2 * g + 1]] for g in range(n_groups) if g != bad_group]
        for g in (0, 2):
            pick = members[2 * g:2 * g + 2]
            c = W.group_circuit([inner.proofs[m] for m in pick], [inner.inputs[m] for m in pick], 3)
            assert np.array_equal(want[0][g], np.array(c.variables, dtype=np.uint32)), g
        for form in FORMS[:-1]:
            with launch_form(ctx, form, n_groups):
                got = _eval_groups(rsv, ctx, wp2, pair, n_groups, inner.fixed, d_own)
            assert all(np.array_equal(a, b) for a, b in zip(want[1:], got[1:])), form
            assert np.array_equal(want[0][good], got[0][good]), form
    finally:
        wp2.close()


def test_groups_bring_their_members_statements(rsv, ctx, inner):
    """copies = 2, two groups of S1 proofs with four different statements: variables 4 and 5 of group g are members 2g and
    2g + 1's, the rows are the oracle's two-member circuits; one rotated statement rejects its group and names the member;
    the chain of the groups is accepted by Chain.verify and by the C oracle under the groups' own statements."""
    cfg = inner.cfg
    wp2 = rsv.WitnessProgram.build(inner.proofs[0], cfg, inner.inputs[0], copies=2, n_fixed=3)
    try:
        assert wp2.inputs()[:2] == (3, 1) and wp2.num_input == 5
        pair = _upload(rsv, inner.proofs[:4])
        own = inner.own[:4].contiguous()
        variables, acc, macc, mreason = _eval_groups(rsv, ctx, wp2, pair, 2, inner.fixed, own)
        assert acc.tolist() == [1, 1] and macc.tolist() == [[1, 1], [1, 1]] and mreason.tolist() == [[0, 0], [0, 0]]
        assert variables[:, 4:6, 0].tolist() == [[11, 12], [13, 14]]
        for g in range(2):
            c = W.group_circuit(inner.proofs[2 * g:2 * g + 2], inner.inputs[2 * g:2 * g + 2], 3)
            assert c.num_input == 5 and np.array_equal(variables[g], np.array(c.variables, dtype=np.uint32)), g
        rec = u32(own).copy()
        rec[3, 0, 1] = 11                                    # member 1 of group 1 under proof 0's statement
        _, acc, macc, mreason = _eval_groups(rsv, ctx, wp2, pair, 2, inner.fixed, _dev(rec))
        assert acc.tolist() == [1, 0] and macc.tolist() == [[1, 1], [1, 0]] and mreason.tolist() == [[0, 0], [0, R_LOGUP]]
        ch = rsv.Chain(ctx, wp2, 2, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, device=DEV,
                       aggregate=True)
        ch.witness(pair, inner.fixed, d_inputs=own)
        ctx.synchronize()
        assert u32(ch.inputs())[:, 3:].tolist() == [[[4, 11 + 2 * g, 0, 0, 0], [5, 12 + 2 * g, 0, 0, 0]] for g in range(2)]
        _finish(ch, cfg)
        acc, reason = ch.verify(cfg)
        ctx.synchronize()
        assert acc.cpu().tolist() == [1, 1] and reason.cpu().tolist() == [0, 0]
        for g, proof in enumerate(ch.proofs()):
            own_g = inner.fixed + [(4, (11 + 2 * g, 0, 0, 0)), (5, (12 + 2 * g, 0, 0, 0))]
            assert [int(x[0]) for x in ob.verify_batch([proof], cfg, own_g)] == [1, 0]
            other = inner.fixed + [(4, (12 + 2 * g, 0, 0, 0)), (5, (11 + 2 * g, 0, 0, 0))]
            assert int(ob.verify_batch([proof], cfg, other)[0][0]) == 0
    finally:
        wp2.close()


# ---------------------------------------------------------------- 6. the C++ example
def test_the_example_recurses_over_two_statements(tmp_path):
    """examples/multi_proofs.cpp --own-inputs through the host layer (WitnessProgram::build_inputs, rsv_witness_eval_inputs):
    level10-1.bin and level11-1.bin, two proofs of one shape, each with the record (1, v) as its own input — under v = 1,
    their statement, both are accepted and variable 4 is 1; under v = 2 the second is rejected at the logup balance."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc, proofs = os.path.join(root, "recursive-stwo_amd", "csrc"), os.path.join(root, "tests", "golden", "proofs")
    exe = os.path.join(str(tmp_path), "multi_proofs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "examples", "multi_proofs.cpp"),
                           "-L" + csrc, "-lrsv_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"])
    a, b = os.path.join(proofs, "level10-1.bin"), os.path.join(proofs, "level11-1.bin")
    out = subprocess.run([exe, "--own-inputs", a, b], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and len(lines) == 2 and all("accepted" in l and "variable 4 = 1" in l for l in lines), out.stdout + out.stderr
    out = subprocess.run([exe, "--own-inputs", a, b + ":2"], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 1 and "accepted" in lines[0] and "REJECTED (stage %d)" % R_LOGUP in lines[1], out.stdout + out.stderr
