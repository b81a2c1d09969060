"""The statement digest on the GPU (`-m gpu`): rsv_statement_digest_dev, the kernel alone, in both of its forms, against the
C oracle's hash_node; crafted rows; a tree of statements folded level by level; the refusals."""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import statement_ref as S
from tests.chain_harness import DEV, u32

pytestmark = pytest.mark.gpu

P = S.P
FORMS = {"row": (1 << 26) + 1, "lane": 1}      # statement_row_max: 1 + the largest batch hashed in the row form
SHAPES = [(1, 1), (1, 7), (1, 8), (1, 9), (2, 8), (1, 17), (1, 67), (2, 67)]   # (copies, n_own): T = 1 .. 134, tiles of 32 records


@pytest.fixture(scope="module")
def ctx(rsv):
    c = rsv.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def _digest(ctx, rec, copies, form, with_bad=True):
    """rec uint32[n_groups * copies, n_own, 5] -> (stmt uint32[n_groups, 8, 5], bad uint8[n_groups]); outputs prefilled."""
    import torch
    n_groups, n_own = rec.shape[0] // copies, rec.shape[1]
    d_stmt = torch.full((n_groups, 8, 5), -1, dtype=torch.int32, device=DEV)
    d_bad = torch.full((n_groups,), 7, dtype=torch.uint8, device=DEV) if with_bad else None
    ctx.set_option("statement_row_max", FORMS[form])
    try:
        ctx.statement_digest(_dev(rec), n_groups, copies, n_own, d_stmt, d_bad)
        ctx.synchronize()
    finally:
        ctx.set_option("statement_row_max", 0)
    return u32(d_stmt), (d_bad.cpu().numpy() if with_bad else None)


def _random_records(rnd, n_members, n_own):
    rec = np.zeros((n_members, n_own, 5), np.uint32)
    rec[:, :, 0] = rnd.integers(0, 1 << 32, (n_members, n_own), dtype=np.uint64)   # idx: any u32, not hashed
    rec[:, :, 1] = rnd.integers(0, P, (n_members, n_own))
    return rec


# ---------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("form", ["row", "lane"])
@pytest.mark.parametrize("n_groups", [1, 3, 70])
@pytest.mark.parametrize("copies,n_own", SHAPES)
def test_kernel_against_hash_node(rsv, ctx, form, n_groups, copies, n_own):
    rnd = np.random.default_rng(10000 * n_groups + 100 * copies + n_own)
    rec = _random_records(rnd, n_groups * copies, n_own)
    rec[0, 0, 1] = P - 1
    stmt, bad = _digest(ctx, rec, copies, form)
    want = ob.hash_node(None, rec[:, :, 1].reshape(n_groups, copies * n_own))
    assert bad.tolist() == [0] * n_groups
    assert np.array_equal(stmt[:, :, 1], want)
    assert np.array_equal(stmt[:, :, 0], np.tile(4 + np.arange(8, dtype=np.uint32), (n_groups, 1))) and not stmt[:, :, 2:].any()
    assert stmt[0, :, 1].tolist() == S.digest(rec[:copies, :, 1].reshape(-1))      # the restated sponge agrees with the oracle
    if n_groups == 3:                                                              # d_bad is optional
        assert np.array_equal(_digest(ctx, rec, copies, form, with_bad=False)[0], stmt)


@pytest.mark.parametrize("form", ["row", "lane"])
def test_kernel_crafted_rows(rsv, ctx, form):
    """T = 2 x 35 = 70 words, three tiles.  Group by group: a value word = P in the first tile; = 0xffffffff in the last
    chunk; a non-zero word 1, 2, 3 of a value; both faults in one group.  Between them untouched groups, whose digests are
    their own and whose flags stay clear."""
    rnd = np.random.default_rng(7)
    copies, n_own, n_groups = 2, 35, 9
    rec = _random_records(rnd, n_groups * copies, n_own)
    rec[2 * 1 + 0, 3, 1] = P
    rec[2 * 3 + 1, 34, 1] = 0xFFFFFFFF
    rec[2 * 4 + 0, 0, 2] = 1
    rec[2 * 5 + 1, 20, 3] = P
    rec[2 * 6 + 1, 33, 4] = 0xFFFFFFFF
    rec[2 * 7 + 0, 9, 1], rec[2 * 7 + 1, 9, 4] = P + 1, 5
    want_bad = [0, 1, 0, 1, 1, 1, 1, 1, 0]
    stmt, bad = _digest(ctx, rec, copies, form)
    want, model_bad = S.statement_records(rec, copies)
    assert model_bad.tolist() == want_bad and bad.tolist() == want_bad
    assert np.array_equal(stmt, want)
    # the offending value word counts as 0: the digest of the same group with the word cleared
    clean = rec.copy()
    clean[:, :, 1][clean[:, :, 1] >= P] = 0
    clean[:, :, 2:] = 0
    stmt_clean, bad_clean = _digest(ctx, clean, copies, form)
    assert np.array_equal(stmt_clean, stmt) and not bad_clean.any()
    assert np.array_equal(stmt[:, :, 1], ob.hash_node(None, clean[:, :, 1].reshape(n_groups, copies * n_own)))
    # a group's digest does not depend on its neighbours: every group alone
    for g in (0, 1, 3, 7, 8):
        solo, solo_bad = _digest(ctx, rec[2 * g:2 * g + 2], copies, form)
        assert np.array_equal(solo[0], want[g]) and solo_bad.tolist() == [want_bad[g]]


def test_a_tree_of_statements_folds_to_eight_words(rsv, ctx):
    """The consumer's use: 64 leaf statements of three records, folded four at a time, level by level, d_stmt of one level
    being d_pi (n_own = 8) of the next (T = 32: remain == 0) — one statement of eight records at the root, whatever the
    depth.  Both forms give the same tree."""
    rnd = np.random.default_rng(11)
    leaves = _random_records(rnd, 64, 3)
    roots = {}
    for form in FORMS:
        level, copies_n_own = leaves, 3
        while level.shape[0] > 1:
            stmt, bad = _digest(ctx, level, 4, form)
            assert not bad.any() and stmt.shape == (level.shape[0] // 4, 8, 5)
            assert np.array_equal(stmt[:, :, 1], ob.hash_node(None, level[:, :, 1].reshape(-1, 4 * copies_n_own)))
            level, copies_n_own = stmt, 8
        roots[form] = level
    assert np.array_equal(roots["row"], roots["lane"]) and roots["row"].shape == (1, 8, 5)


# ---------------------------------------------------------------- 2. refusals before any device work
def test_refusals_leave_the_outputs_alone(rsv, ctx):
    import torch
    rec = _random_records(np.random.default_rng(3), 6, 4)
    d_rec = _dev(rec)
    d_stmt = torch.full((3, 8, 5), -1, dtype=torch.int32, device=DEV)
    d_bad = torch.full((3,), 7, dtype=torch.uint8, device=DEV)

    def code(call):
        with pytest.raises(rsv.RsvError) as e:
            call()
        return e.value.code

    E_NULL, E_SIZE = -1, -2
    assert code(lambda: ctx.statement_digest(None, 3, 2, 4, d_stmt, d_bad)) == E_NULL
    assert code(lambda: ctx.statement_digest(d_rec, 3, 2, 4, None, d_bad)) == E_NULL
    for copies, n_own in ((0, 4), (65, 4), (2, 0), (2, 4097)):
        assert code(lambda: ctx.statement_digest(d_rec, 3, copies, n_own, d_stmt, d_bad)) == E_SIZE, (copies, n_own)
    assert code(lambda: ctx.statement_digest(d_rec, (1 << 26) + 1, 2, 4, d_stmt, d_bad)) == E_SIZE
    assert code(lambda: ctx.statement_digest(d_rec, 1 << 20, 64, 4096, d_stmt, d_bad)) == E_SIZE      # beyond RSV_MAX_INPUT_RECORDS
    assert rsv.lib.rsv_statement_digest_dev(ctx._h, d_rec.data_ptr() + 2, 3, 2, 4, d_stmt.data_ptr(), d_bad.data_ptr()) == E_SIZE
    assert rsv.lib.rsv_statement_digest_dev(None, d_rec.data_ptr(), 3, 2, 4, d_stmt.data_ptr(), d_bad.data_ptr()) == E_NULL
    ctx.statement_digest(None, 0, 2, 4, None, None)                                                   # an empty batch is no error
    ctx.synchronize()
    assert (u32(d_stmt) == 0xFFFFFFFF).all() and (d_bad.cpu().numpy() == 7).all()


# ================================================================ the hashed program (rsv_witness_program_build_inputs_hashed)
# The inner proofs are tests/test_witness_inputs_gpu.py's: circuit S1 under CONFIG, witness i with the statement 11 + i,
# proved by the chain itself (a witness that draws a duplicate query is made again from another seed).
from tests import witness_inputs_ref as W                                                    # noqa: E402
from tests.chain_harness import FILL, LAUNCH_FORMS_FEW as LAUNCH_FORMS, launch_form          # noqa: E402
from tests.test_witness_inputs_gpu import N, _dev as _dev_any, _finish, _full, _upload, inner  # noqa: E402,F401

R_PARSE, R_LOGUP, R_DUP_QUERY = 1, 3, 5
E_NULL, E_SIZE, E_RANGE = -1, -2, -5


@pytest.fixture(scope="module")
def hashed(rsv, inner):
    """The hashed programs of the S1 shape: one copy and two."""
    class H:
        pass
    h = H()
    h.wp = rsv.WitnessProgram.build(inner.proofs[0], inner.cfg, inner.inputs[0], n_fixed=3, hashed=True)
    h.wp2 = rsv.WitnessProgram.build(inner.proofs[0], inner.cfg, inner.inputs[0], copies=2, n_fixed=3, hashed=True)
    yield h
    h.wp.close()
    h.wp2.close()


def _eval_hashed(ctx, wp, pair, n_groups, fixed, d_own, layout="by_proof", form=(0, 0, 0), pace=None):
    """The evaluating call of a hashed program (copies 1: Context.witness, else witness_groups), outputs prefilled ->
    (variables [n_groups, n_vars, 4], member flow [n_groups * m, F, 32], tail [n_groups, S, 32], swap bytes, accept,
    member accept, member reason).  pace: "row" / "lane" forces that form of the digest kernel, which here writes the hash's
    flow records (k_statement_digest<.., true>); None: the default rule, the row form at these sizes."""
    m, F, S_ = wp.shape.copies, wp.shape.flow_count, wp.stmt_flow
    by_variable = layout == "by_variable"
    total = n_groups * (m * F + S_)
    d_vars = _full((wp.n_vars, n_groups, 4) if by_variable else (n_groups, wp.n_vars, 4))
    d_flow, d_swap, d_acc = _full((total, 32)), _full((total,), True), _full((n_groups,), True)
    d_macc, d_mreason = _full((n_groups * m,), True), _full((n_groups * m,), True)
    ctx.set_option("witness_layout", layout)
    ctx.set_option("statement_row_max", FORMS[pace] if pace else 0)
    try:
        with launch_form(ctx, form, n_groups):
            if m == 1:
                ctx.witness(wp, *pair, n_groups, d_vars, d_acc, d_mreason, inputs=fixed, d_flow=d_flow, d_flow_swap=d_swap, d_inputs=d_own)
                ctx.synchronize()
                d_macc = d_acc
            else:
                ctx.witness_groups(wp, *pair, n_groups, d_vars, d_acc, d_macc, d_mreason, inputs=fixed, d_flow=d_flow, d_flow_swap=d_swap, d_inputs=d_own)
                ctx.synchronize()
    finally:
        ctx.set_option("witness_layout", "by_proof")
        ctx.set_option("statement_row_max", 0)
    v, flow = u32(d_vars), u32(d_flow)
    cut = n_groups * m * F
    return ((v.transpose(1, 0, 2) if by_variable else v), flow[:cut].reshape(n_groups * m, F, 32), flow[cut:].reshape(n_groups, S_, 32),
            d_swap.cpu().numpy(), d_acc.cpu().numpy(), d_macc.cpu().numpy(), d_mreason.cpu().numpy())


_ORACLE = {}


def _oracle_rows(inner, members):
    key = tuple(members)
    if key not in _ORACLE:
        c = S.group_circuit([inner.proofs[m] for m in members], [inner.inputs[m] for m in members], 3)
        assert c.num_input == 11
        _ORACLE[key] = np.array(c.variables, dtype=np.uint32)
    return _ORACLE[key]


def test_the_hashed_program_reports_itself(rsv, inner, hashed):
    for wp, m in ((hashed.wp, 1), (hashed.wp2, 2)):
        assert wp.statement() == (True, 8, 2) and wp.stmt_flow == 2 and wp.num_input == 11 and wp.inputs()[:2] == (3, 1)
        prog, F = wp.export(), wp.shape.flow_count
        assert prog.flow_wires.shape == (m * F + 2, 5)
        by_dst = prog.instr[np.argsort(prog.instr[:, 1])]
        assert by_dst[4:12, 0].tolist() == [S.W_STMT] * 8 and by_dst[12:12 + m, 0].tolist() == [S.W_INPUT] * m
        tail = prog.instr[(prog.instr[:, 0] == 11) & (prog.instr[:, 4] >= m * F)]
        assert len(tail) == 4 and set(tail[:, 4].tolist()) == {m * F, m * F + 1}
        rows, _ = wp.gates()
        assert all(rows[v].tolist() == [v, 0, v, 1, 0, 1] for v in range(4, 12 + m))
    assert inner.wp.statement() == (False, 0, 0)
    # the arrays of a hashed program are for reading: a program made from them would have no tail to load the hash from
    exported = hashed.wp.export()
    for refused in (lambda: exported.save("unused.npz"), lambda: exported.save_raw("unused.bin"), lambda: rsv.WitnessProgram(exported)):
        with pytest.raises(ValueError, match="hashed"):
            refused()
    ch = rsv.Chain(rsv.Context(0), hashed.wp, 1, inner.cfg.log_blowup_factor, log_last=inner.cfg.log_last_layer_degree_bound, device=DEV)
    with pytest.raises(ValueError, match="hashed"):
        ch.load(np.zeros((1, hashed.wp.n_vars, 4), np.uint32))


@pytest.mark.parametrize("layout", ["by_proof", "by_variable"])
@pytest.mark.parametrize("n", [1, 3, N])
def test_hashed_rows_are_the_oracles_variables(rsv, ctx, inner, hashed, n, layout):
    """n proofs with their own statements through the hashed program: every proof accepted, variables 4 .. 11 of row i are
    the digest of (11 + i), variable 12 is 11 + i; the rows of the first three are the oracle's, word for word; the members'
    flow is the program's without the hash, the tail holds the hash's records; the reference's two checks pass."""
    import torch
    wp = hashed.wp
    pair = _upload(rsv, inner.proofs[:n])
    own = inner.own[:n].contiguous()
    variables, flow, tail, swap, acc, _, reason = _eval_hashed(ctx, wp, pair, n, inner.fixed, own, layout)
    assert acc.tolist() == [1] * n and reason.tolist() == [0] * n, reason.tolist()
    assert variables[:, 12].tolist() == [[11 + i, 0, 0, 0] for i in range(n)]
    assert variables[:, 4:12, 0].tolist() == [S.digest([11 + i]) for i in range(n)] and not variables[:, 4:12, 1:].any()
    for i in range(min(n, 3)):
        want = _oracle_rows(inner, [i])
        assert variables[i].shape == want.shape and np.array_equal(variables[i], want), i
    assert np.array_equal(tail, np.stack([S.flow_records([11 + i]) for i in range(n)])) and not swap[n * wp.shape.flow_count:].any()
    from tests.test_witness_inputs_gpu import _eval
    plain = _eval(rsv, ctx, inner.wp, pair, n, inner.fixed, own, layout)
    assert np.array_equal(flow, plain[1]) and np.array_equal(swap[:n * wp.shape.flow_count].reshape(n, -1), plain[2])
    # check_arithmetics and check_poseidon_invocations on the result: the flow of a witness in the circuit's own order
    d_vars = _dev(variables)
    d_flow = _dev(np.concatenate([flow, tail], axis=1))
    d_swap = torch.from_numpy(np.concatenate([swap[:n * wp.shape.flow_count].reshape(n, -1), np.zeros((n, 2), np.uint8)], axis=1)).to(DEV)
    before = d_flow.clone()
    ok, bad_row, bad_flow = torch.ones(n, dtype=torch.uint8, device=DEV), _full((n,)), _full((n,))
    ctx.circuit_check(wp, d_vars, n, ok, bad_row)
    ctx.circuit_flow(wp, d_vars, n, d_flow, d_swap, ok, bad_flow)
    ctx.synchronize()
    assert ok.cpu().tolist() == [1] * n and u32(bad_row).tolist() == [0xFFFFFFFF] * n and u32(bad_flow).tolist() == [0xFFFFFFFF] * n
    assert torch.equal(before, d_flow)


def _outer_chain(rsv, ctx, wp, cfg, pair, fixed, d_own, n, aggregate=False):
    """Chain.witness .. fri_open .. verify of n outer proofs (groups with aggregate) -> an object with what the tests ask of."""
    import torch

    class O:
        pass
    o = O()
    o.n = n
    o.ch = rsv.Chain(ctx, wp, n, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, device=DEV,
                     aggregate=aggregate)
    o.ch.witness(pair, fixed, d_inputs=d_own)
    ctx.synchronize()
    o.witness_acc = o.ch.acc.cpu().tolist()
    o.statements = o.ch.inputs()
    _finish(o.ch, cfg)
    o.ok = o.ch.numpy()["ok"].tolist()
    acc, reason = o.ch.verify(cfg)
    ctx.synchronize()
    o.acc, o.reason = acc.cpu().tolist(), reason.cpu().tolist()
    o.proofs, o.packed = o.ch.proofs(), o.ch.pack()
    torch.cuda.synchronize()
    return o


@pytest.fixture(scope="module")
def outer(rsv, ctx, inner, hashed):
    """Three outer proofs of the hashed program that verify.  Under nine queries a proof draws a query position twice now and
    then, which every verifier rejects (RSV_R_DUP_QUERY); the inner fixture makes such a witness again from another seed, and an
    outer proof is a function of its inner proof alone, so here the inner proofs are CHOSEN: the first eight are taken through
    the outer chain once (`wide`: nothing but a duplicate query may reject one), and the first three whose outer proofs
    verify make the chain the tests are about."""
    wide = _outer_chain(rsv, ctx, hashed.wp, inner.cfg, (inner.d_blob, inner.d_offsets[:9].contiguous()), inner.fixed,
                        inner.own[:8].contiguous(), 8)
    assert all((a, r) in ((1, 0), (0, R_DUP_QUERY)) for a, r in zip(wide.acc, wide.reason)), (wide.acc, wide.reason)
    pick = [i for i in range(8) if wide.acc[i]][:3]
    assert len(pick) == 3, wide.acc
    own = inner.own[pick].contiguous()
    o = _outer_chain(rsv, ctx, hashed.wp, inner.cfg, _upload(rsv, [inner.proofs[i] for i in pick]), inner.fixed, own, 3)
    o.own, o.pick, o.wide = own, pick, wide
    return o


def _records(r):
    return [(int(k), tuple(int(x) for x in v)) for k, *v in np.asarray(r).tolist()]


def test_the_loop_closes_on_eight_words(rsv, ctx, inner, outer):
    """The outer chain of the hashed program: its statements are the digests of the inner ones, Chain.verify accepts all three,
    the C oracle accepts each outer proof under its eleven records, and with the digests rotated by one proof every proof is
    rejected at the logup balance, as the oracle rejects it."""
    import torch
    n, cfg, statements = outer.n, inner.cfg, outer.statements
    assert outer.witness_acc == [1] * n and outer.ok == [1] * n
    assert tuple(statements.shape) == (n, 11, 5)
    d_stmt = torch.full((n, 8, 5), -1, dtype=torch.int32, device=DEV)
    ctx.statement_digest(outer.own, n, 1, 1, d_stmt)
    ctx.synchronize()
    assert torch.equal(statements[:, 3:], d_stmt)
    assert u32(statements)[:, 3:, 1].tolist() == [S.digest([11 + i]) for i in outer.pick]
    assert u32(statements)[:, :3].tolist() == [[[1, 1, 0, 0, 0], [2, 0, 1, 0, 0], [3, 0, 0, 1, 0]]] * n
    assert outer.acc == [1] * n and outer.reason == [0] * n, (outer.acc, outer.reason)
    rec = u32(statements)
    d_rot = torch.cat([statements[:, :3], statements[:, 3:].roll(-1, 0)], dim=1).contiguous()
    d_acc, d_reason = _full((n,), True), _full((n,), True)
    ctx.verify_batch(*outer.packed, n, d_acc, d_reason, cfg=cfg, d_inputs=d_rot, n_inputs=11)
    ctx.synchronize()
    assert d_acc.cpu().tolist() == [0] * n and d_reason.cpu().tolist() == [R_LOGUP] * n
    for i in range(n):
        assert [int(x[0]) for x in ob.verify_batch([outer.proofs[i]], cfg, _records(rec[i]))] == [1, 0], i
        rotated = np.concatenate([rec[i, :3], rec[(i + 1) % n, 3:]])
        assert [int(x[0]) for x in ob.verify_batch([outer.proofs[i]], cfg, _records(rotated))] == [0, R_LOGUP], i
    # the proofs of the choosing pass: each has the C oracle's verdict
    wrec = u32(outer.wide.statements)
    for i in range(outer.wide.n):
        assert [int(x[0]) for x in ob.verify_batch([outer.wide.proofs[i]], cfg, _records(wrec[i]))] == [outer.wide.acc[i], outer.wide.reason[i]], i


@pytest.mark.parametrize("pace", ["row", "lane"])
def test_both_forms_of_the_kernel_write_the_hash_records(rsv, ctx, inner, hashed, pace):
    """The evaluating calls run the digest kernel in the form that also writes the flow records, in the row form below the
    crossover and a lane per group above it: both are forced here, for three proofs (T = 1) and for three groups of two
    (T = 2).  The tail holds the restated sponge's (left, right, out) states, its swap bytes are 0, variables 4 .. 11 are the
    digest, and the rows are the oracle's.  (T = 16 and T = 67: the second-level and the many-records tests, below.)"""
    n = 3
    for wp, m in ((hashed.wp, 1), (hashed.wp2, 2)):
        members = [m * g + c for g in range(n) for c in range(m)]
        pair = _upload(rsv, [inner.proofs[k] for k in members])
        d_own = inner.own[members].contiguous()
        variables, flow, tail, swap, acc, macc, mreason = _eval_hashed(ctx, wp, pair, n, inner.fixed, d_own, pace=pace)
        assert acc.tolist() == [1] * n and macc.tolist() == [1] * (n * m) and mreason.tolist() == [0] * (n * m)
        words = [[11 + members[m * g + c] for c in range(m)] for g in range(n)]
        assert np.array_equal(tail, np.stack([S.flow_records(w) for w in words]))
        cut = n * m * wp.shape.flow_count
        assert swap.shape == (cut + 2 * n,) and not swap[cut:].any()
        assert variables[:, 4:12, 0].tolist() == [S.digest(w) for w in words] and not variables[:, 4:12, 1:].any()
        for g in range(n):
            assert np.array_equal(variables[g], _oracle_rows(inner, members[m * g:m * g + m])), (m, g)
        other = _eval_hashed(ctx, wp, pair, n, inner.fixed, d_own)
        assert all(np.array_equal(a, b) for a, b in zip(other, (variables, flow, tail, swap, acc, macc, mreason))), m


@pytest.mark.parametrize("n", [3, N])
def test_every_launch_form_of_the_hashed_program(rsv, ctx, inner, hashed, n):
    """By the default rule batches this small run the whole program in one launch (k_witness_small over WitnessStmtArgs / WitnessGroupStmtArgs): the other
    instantiations over WitnessStmtArgs and WitnessGroupStmtArgs — the level kernels below and from 64 rows on, the strip, the
    one-launch tail — are forced through the options at 3 and 70, for proofs and for groups of two (group g = proofs 2g and
    2g + 1 of the 70, taken round again).  One record has a non-zero word 2: its proof, or its group, is rejected
    (RSV_R_PARSE on the member).  Under every form: the verdicts and every byte of the default form's outputs for the accepted
    rows; under the default form the oracle's rows."""
    for wp, m in ((hashed.wp, 1), (hashed.wp2, 2)):
        members = [(m * g + c) % N for g in range(n) for c in range(m)]
        pair = _upload(rsv, [inner.proofs[k] for k in members])
        rec = u32(inner.own)[members].copy()
        bad = 1 if n == 3 else 64
        rec[m * bad + m - 1, 0, 3] = 1
        d_own = _dev(rec)
        good = np.arange(n) != bad
        want = _eval_hashed(ctx, wp, pair, n, inner.fixed, d_own)
        assert want[4].tolist() == good.astype(int).tolist()
        assert want[5].reshape(n, m)[bad].tolist() == [1] * (m - 1) + [0] and want[6].reshape(n, m)[bad, m - 1] == R_PARSE
        assert want[0][good][:, 12:12 + m, 0].tolist() == [[11 + members[m * g + c] for c in range(m)] for g in range(n) if g != bad]
        assert want[0][good][:, 4:12, 0].tolist() == [S.digest([11 + members[m * g + c] for c in range(m)]) for g in range(n) if g != bad]
        for g in (0, 2):
            assert np.array_equal(want[0][g], _oracle_rows(inner, members[m * g:m * g + m])), (m, g)
        assert np.array_equal(want[2][good], np.stack([S.flow_records([11 + members[m * g + c] for c in range(m)]) for g in range(n) if g != bad]))
        for form in LAUNCH_FORMS[:-1]:
            got = _eval_hashed(ctx, wp, pair, n, inner.fixed, d_own, form=form)
            assert all(np.array_equal(a, b) for a, b in zip(want[4:], got[4:])), (m, form)
            assert np.array_equal(want[0][good], got[0][good]) and np.array_equal(want[2][good], got[2][good]), (m, form)
            assert np.array_equal(want[1], got[1]), (m, form)


def test_many_records_through_a_hashed_program(rsv, ctx):
    """Two witnesses of a circuit with 70 public inputs (n_own = 67: nine chunks, remainder 3, three tiles of the kernel),
    proved by the chain, through a hashed program: in both forms of the digest kernel the rows are the oracle's, the statement is
    the digest of the 67 words and the tail holds the hash's ten records; the loop closes — both outer proofs are accepted by
    Chain.verify and by the C oracle under their eleven records, and rejected under each other's digests.  A witness whose
    inner or outer proof draws a query position twice is made again from another seed (as tests/test_witness_inputs_gpu.py's)."""
    from tests import verify_inputs_ref as V
    from tests.test_verify_inputs_gpu import _chain_of
    seeds, circ, wp, outer_ = [1, 2], None, None, None
    try:
        for _ in range(6):
            builts = [V.build_many(70, first=11, seed=seeds[0]), V.build_many(70, first=9000, seed=seeds[1], bit=0)]
            if circ is None:
                circ = rsv.Circuit(builts[0].gates, builts[0].flow_wires, builts[0].n_vars, 70, builts[0].witness_ops)
            ch, cfg = _chain_of(rsv, ctx, circ, builts)
            _finish(ch, cfg)
            acc, reason = ch.verify(cfg)
            ctx.synchronize()
            acc, reason = acc.cpu().tolist(), reason.cpu().tolist()
            assert all((a, r) in ((1, 0), (0, R_DUP_QUERY)) for a, r in zip(acc, reason)), (acc, reason)
            if all(acc):
                proofs, inputs, pair = ch.proofs(), [b.inputs for b in builts], ch.pack()
                own = ch.inputs()[:, 3:].contiguous()
                if wp is not None:
                    wp.close()
                wp = rsv.WitnessProgram.build(proofs[0], cfg, inputs[0], n_fixed=3, hashed=True)
                outer_ = _outer_chain(rsv, ctx, wp, cfg, pair, inputs[0][:3], own, 2)
                acc, reason = outer_.acc, outer_.reason
                assert all((a, r) in ((1, 0), (0, R_DUP_QUERY)) for a, r in zip(acc, reason)), (acc, reason)
                if all(acc):
                    break
            seeds = [sd if ok else sd + 100 for sd, ok in zip(seeds, acc)]
        assert outer_ is not None and outer_.acc == [1, 1] and outer_.reason == [0, 0], seeds
        assert wp.statement() == (True, 8, 10) and wp.num_input == 11 and wp.inputs()[:2] == (3, 67)
        for pace in ("row", "lane"):
            variables, _, tail, swap, acc, _, reason = _eval_hashed(ctx, wp, pair, 2, inputs[0][:3], own, pace=pace)
            assert acc.tolist() == [1, 1] and reason.tolist() == [0, 0] and not swap[2 * wp.shape.flow_count:].any()
            for i in range(2):
                words = [int(v[0]) for _, v in inputs[i][3:]]
                c = S.group_circuit([proofs[i]], [inputs[i]], 3)
                assert np.array_equal(variables[i], np.array(c.variables, dtype=np.uint32)), (pace, i)
                assert variables[i, 4:12, 0].tolist() == S.digest(words) and np.array_equal(tail[i], S.flow_records(words)), (pace, i)
        rec = u32(outer_.statements)
        assert rec.shape == (2, 11, 5) and outer_.witness_acc == [1, 1] and outer_.ok == [1, 1]
        for i, proof in enumerate(outer_.proofs):
            assert [int(x[0]) for x in ob.verify_batch([proof], cfg, _records(rec[i]))] == [1, 0], i
            assert [int(x[0]) for x in ob.verify_batch([proof], cfg, _records(np.concatenate([rec[i, :3], rec[1 - i, 3:]])))] == [0, R_LOGUP], i
    finally:
        if wp is not None:
            wp.close()
        if circ is not None:
            circ.close()


def test_the_statement_keeps_its_size_at_the_second_level(rsv, ctx, inner, outer):
    """A second-level hashed program built on a first-level outer proof, its eight digest records the own inputs (n_own = 8),
    with two copies: T = 16, two full chunks.  A group of two first-level proofs, in both forms of the digest kernel: the witness
    passes the reference's arithmetic check, its statement is again eight words — the digest kernel applied to the first level's
    statements —, the tail holds the hash's three records, and num_input stays 11.  Then that level is proved too: the chain of
    the group is accepted by Chain.verify and by the C oracle under its eleven records (a pair whose proof draws a query
    position twice gives way to the next pair of first-level proofs)."""
    import time
    import torch
    cfg = inner.cfg
    rec = u32(outer.statements)
    inputs = _records(rec[0])
    wp = rsv.WitnessProgram.build(outer.proofs[0], cfg, inputs, copies=2, n_fixed=3, hashed=True)
    try:
        assert wp.statement() == (True, 8, 3) and wp.num_input == 11 and wp.inputs()[:2] == (3, 8)
        level2 = None
        for good in ([0, 1], [1, 2], [2, 0]):
            pair = _upload(rsv, [outer.proofs[i] for i in good])
            d_own = outer.statements[good][:, 3:].contiguous()
            words = rec[good][:, 3:, 1].reshape(-1).tolist()
            d_stmt = torch.full((1, 8, 5), -1, dtype=torch.int32, device=DEV)
            ctx.statement_digest(d_own, 1, 2, 8, d_stmt)
            ctx.synchronize()
            for pace in ("row", "lane"):
                variables, _, tail, swap, acc, macc, mreason = _eval_hashed(ctx, wp, pair, 1, inputs[:3], d_own, pace=pace)
                assert acc.tolist() == [1] and macc.tolist() == [1, 1] and mreason.tolist() == [0, 0]
                assert u32(d_stmt)[0, :, 1].tolist() == S.digest(words) == variables[0, 4:12, 0].tolist()
                assert variables[0, 12:28, 0].tolist() == words and np.array_equal(tail[0], S.flow_records(words))
                assert not swap[2 * wp.shape.flow_count:].any()
                ok, bad_row = torch.ones(1, dtype=torch.uint8, device=DEV), _full((1,))
                ctx.circuit_check(wp, _dev(variables), 1, ok, bad_row)
                ctx.synchronize()
                assert ok.cpu().tolist() == [1] and u32(bad_row).tolist() == [0xFFFFFFFF]
            t0 = time.perf_counter()
            level2 = _outer_chain(rsv, ctx, wp, cfg, pair, inputs[:3], d_own, 1, aggregate=True)
            print("second level: witness .. verify of one group of two in %.2f s" % (time.perf_counter() - t0))
            assert (level2.acc[0], level2.reason[0]) in ((1, 0), (0, R_DUP_QUERY))
            if level2.acc[0]:
                break
        assert level2.acc == [1] and level2.reason == [0] and level2.witness_acc == [1] and level2.ok == [1]
        top = u32(level2.statements)
        assert top.shape == (1, 11, 5) and np.array_equal(top[0, 3:], u32(d_stmt)[0])
        assert [int(x[0]) for x in ob.verify_batch([level2.proofs[0]], cfg, _records(top[0]))] == [1, 0]
    finally:
        wp.close()


def test_hashed_refusals_come_before_any_device_work(rsv, ctx, inner, hashed):
    """A hashed program with d_pi == NULL, with another n_own, through the calls without inputs, of two copies through the
    call for proofs; n_own == 0 at build.  RSV_E_NULL / RSV_E_SIZE, and not one output byte changes."""
    import ctypes
    import torch
    lib, wp, n = rsv.lib, hashed.wp, 3
    F = wp.shape.flow_count
    pair = _upload(rsv, inner.proofs[:n])
    d_own = inner.own[:n].contiguous()
    two = torch.cat([d_own, d_own], dim=1).contiguous()
    outs = [_full((n, wp.n_vars, 4)), _full((n * (F + 2), 32)), _full((n * (F + 2),), True), _full((n,), True), _full((n,), True)]
    pc = ctx.prepare_cfg(wp.cfg(), n)
    fixed = rsv.make_inputs(inner.fixed)

    def call(d_pi=d_own.data_ptr(), n_own=1, prog=wp._h):
        ctx.acquire_from_torch()
        return lib.rsv_witness_eval_inputs_dev(ctx._h, prog, pair[0].data_ptr(), pair[1].data_ptr(), n, pc.ref(), fixed, 3, d_pi, n_own,
                                               outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr())
    assert call(d_pi=None) == E_NULL
    assert call(d_pi=two.data_ptr(), n_own=2) == E_SIZE and call(n_own=0) == E_SIZE
    assert call(prog=hashed.wp2._h) == E_SIZE                                     # two copies hash a group's statements
    for program in (hashed.wp, hashed.wp2):
        with pytest.raises(rsv.RsvError) as e:                                    # the calls without per-proof inputs
            ctx.witness(program, *pair, n, outs[0], outs[3], outs[4], inputs=inner.inputs[0])
        assert e.value.code == E_SIZE
    with pytest.raises(rsv.RsvError) as e:
        ctx.witness_groups(hashed.wp2, *pair, 1, outs[0], outs[3], outs[3], outs[4], inputs=inner.inputs[0])
    assert e.value.code == E_SIZE
    with pytest.raises(rsv.RsvError) as e:                                        # n_own == 0 at build
        rsv.WitnessProgram.build(inner.proofs[0], inner.cfg, inner.inputs[0], n_fixed=4, hashed=True)
    assert e.value.code == E_SIZE
    with pytest.raises(ValueError):
        rsv.WitnessProgram.build(inner.proofs[0], inner.cfg, inner.inputs[0], hashed=True)
    assert lib.rsv_witness_program_statement(None, None, None, None) == E_NULL
    ctx.synchronize()
    for t in outs:
        assert bool((t == (0xFF if t.dtype == torch.uint8 else -1)).all())
    assert call() == 0                                                            # and the same arguments, unchanged, are taken
    ctx.synchronize()
    assert outs[3].cpu().tolist() == [1] * n


def test_the_example_hashes_its_statements(tmp_path):
    """examples/multi_proofs.cpp --hash-inputs through the host layer (WitnessProgram::build_inputs_hashed,
    rsv_witness_eval_inputs): level10-1.bin and level11-1.bin, each with the record (1, 1) as its own input — both accepted,
    variable 12 is the record and variables 4 .. 11 the digest of (1); under (1, 2) the second is rejected at the logup balance."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc, proofs = os.path.join(root, "recursive-stwo_amd", "csrc"), os.path.join(root, "tests", "golden", "proofs")
    exe = os.path.join(str(tmp_path), "multi_proofs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "examples", "multi_proofs.cpp"),
                           "-L" + csrc, "-lrsv_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"])
    a, b = os.path.join(proofs, "level10-1.bin"), os.path.join(proofs, "level11-1.bin")
    out = subprocess.run([exe, "--hash-inputs", a, b], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    want = "variable 12 = 1, statement = " + " ".join(str(w) for w in S.digest([1]))
    assert out.returncode == 0 and len(lines) == 2 and all("accepted" in l and l.endswith(want) for l in lines), out.stdout + out.stderr
    out = subprocess.run([exe, "--hash-inputs", a, b + ":2"], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 1 and "accepted" in lines[0] and "REJECTED (stage %d)" % R_LOGUP in lines[1], out.stdout + out.stderr
