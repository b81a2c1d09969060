"""Aggregation (`-m gpu`): a circuit of `copies` copies of the verifier in which every copy verifies its OWN proof
(rsv_witness_eval_groups_dev, rsv_witness_trace_groups_dev, Chain(aggregate=True)).  A = level10-1.bin and B = level11-1.bin
have one shape and one configuration; the program is built from A with copies = 2.  The expected values are the oracle's
circuit of a group (tests/aggregate_ref.py, pinned by tests/test_aggregate_host.py); the same-proof group is pinned to the
existing call, which the reference pins, and five copies of one proof to the reference's own aggregated fixture.  Every
comparison is exact on 32-bit words; outputs are prefilled with 0xffffffff (flags with 0xff)."""
import numpy as np
import pytest

from tests import aggregate_ref as R
from tests import oracle_binding as ob
from tests.aggregate_ref import A, B, COPIES
from tests.chain_harness import DEV, FILL, LAUNCH_FORMS, inputs_of, launch_form, pin_of, program_of
from tests.conftest import Cfg, fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
FOREIGN = "level12-1.bin"  # a proof of another shape


@pytest.fixture(scope="module")
def wp(rsv):
    prog = rsv.WitnessProgram.build(read_proof(A), fixture_cfg(A), inputs_of(A), copies=COPIES, set_walks=R.walks())
    yield prog
    prog.close()


def _proofs():
    a = read_proof(A)
    return {"A": a, "B": read_proof(B), "bad": ob.tamper(a, 5), "foreign": read_proof(FOREIGN)}


def _full(shape, dtype):
    import torch
    return torch.full(shape, -1 if dtype is torch.int32 else 255, dtype=dtype, device=DEV)


def _upload(rsv, flat):
    import torch
    blob, offsets = rsv.pack(flat)
    return torch.from_numpy(blob.copy()).to(DEV), torch.from_numpy(offsets.astype(np.int64)).to(DEV)


def _eval(rsv, ctx, wp, groups, by_variable=False, batch=None):
    """Context.witness_groups on groups of kinds -> the device tensors (vars, acc, member_accept, member_reason, flow, swap).
    Synchronises: the uploaded blob lives no longer than this call."""
    import torch
    proofs = _proofs()
    n, m, F = len(groups), wp.shape.copies, wp.shape.flow_count
    d_blob, d_off = batch if batch is not None else _upload(rsv, [proofs[k] for g in groups for k in g])
    d_vars = _full((wp.n_vars, n, 4) if by_variable else (n, wp.n_vars, 4), torch.int32)
    d_acc, d_macc, d_mreason = _full((n,), torch.uint8), _full((n, m), torch.uint8), _full((n, m), torch.uint8)
    d_flow, d_swap = _full((n, m, F, 32), torch.int32), _full((n, m, F), torch.uint8)
    ctx.witness_groups(wp, d_blob, d_off, n, d_vars, d_acc, d_macc, d_mreason, inputs=inputs_of(A), d_flow=d_flow, d_flow_swap=d_swap)
    ctx.synchronize()
    return d_vars, d_acc, d_macc, d_mreason, d_flow, d_swap


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_values_of_mixed_groups(rsv, wp):
    """[A,B], [B,A], [A,A], [A, tamper(A)], [B, a proof of another shape]: the group verdicts, the members' verdicts, the
    `variables` of the three accepted groups against the oracle's circuits of those groups, and every member's slot of the
    flow tensor against the C oracle's PoseidonFlow of that member."""
    groups = [("A", "B"), ("B", "A"), ("A", "A"), ("A", "bad"), ("B", "foreign")]
    want = {g: R.variables(tuple({"A": A, "B": B}[k] for k in g)) for g in groups[:3]}
    assert want[("A", "B")].shape == (wp.n_vars, 4) == (95537, 4)
    assert not np.array_equal(want[("A", "B")], want[("A", "A")]), "the expected vectors of [A,B] and [A,A] are equal: the test says nothing"
    ctx = rsv.Context(0)
    d_vars, d_acc, d_macc, d_mreason, d_flow, d_swap = _eval(rsv, ctx, wp, groups)
    assert d_acc.cpu().tolist() == [1, 1, 1, 0, 0]
    assert d_macc.cpu().tolist() == [[1, 1], [1, 1], [1, 1], [1, 0], [1, 0]]
    reason = d_mreason.cpu().numpy()
    assert not reason[:3].any() and reason[3].tolist()[0] == 0 and reason[3].tolist()[1] != 0 and reason[4, 0] == 0
    got = _u32(d_vars)
    for k, g in enumerate(groups[:3]):
        assert np.array_equal(got[k], want[g]), g
    flow, swap = _u32(d_flow), d_swap.cpu().numpy()
    want_flow = {"A": ob.poseidon_flow(read_proof(A), inputs_of(A)), "B": ob.poseidon_flow(read_proof(B), inputs_of(A))}
    assert len(want_flow["A"]) == wp.shape.flow_count == 3782
    for k, g in enumerate(groups):
        for c, kind in enumerate(g):
            if kind in want_flow:
                assert np.array_equal(flow[k, c], want_flow[kind][:, :32]), (k, c)
                assert np.array_equal(swap[k, c], want_flow[kind][:, 32].astype(np.uint8)), (k, c)
    ctx.close()


def test_one_copy_is_the_existing_call(rsv):
    """copies = 1: the grouped call on [A, B, tamper(A)] writes what rsv_witness_eval_dev writes, in every output."""
    import torch
    wp1 = rsv.WitnessProgram.build(read_proof(A), fixture_cfg(A), inputs_of(A), copies=1, set_walks=R.walks(copies=1))
    kinds = ["A", "B", "bad"]
    n, F = 3, wp1.shape.flow_count
    batch = _upload(rsv, [_proofs()[k] for k in kinds])
    ctx = rsv.Context(0)
    d_vars, d_acc, d_reason = _full((n, wp1.n_vars, 4), torch.int32), _full((n,), torch.uint8), _full((n,), torch.uint8)
    d_flow, d_swap = _full((n, F, 32), torch.int32), _full((n, F), torch.uint8)
    ctx.witness(wp1, *batch, n, d_vars, d_acc, d_reason, inputs=inputs_of(A), d_flow=d_flow, d_flow_swap=d_swap)
    g_vars, g_acc, g_macc, g_mreason, g_flow, g_swap = _eval(rsv, ctx, wp1, [(k,) for k in kinds], batch=batch)
    ctx.synchronize()
    assert d_acc.cpu().tolist() == [1, 1, 0] == g_acc.cpu().tolist() == g_macc[:, 0].cpu().tolist()
    assert torch.equal(d_reason, g_mreason[:, 0]) and d_reason[2] != 0
    assert torch.equal(d_vars, g_vars) and torch.equal(d_flow, g_flow[:, 0]) and torch.equal(d_swap, g_swap[:, 0])
    assert wp1.group_scratch_bytes(n) == wp1.scratch_bytes(n)
    ctx.close()
    wp1.close()


def test_same_proof_group_is_the_existing_path(rsv, wp):
    """[A, A] equals the existing call on [A] under the same 2-copy program (the path the reference pins), in `variables`
    and in the Plonk, Poseidon and ops columns."""
    import torch
    lp, lq = wp.trace_sizes()
    n_ops = len(wp.gates()[1])
    F = wp.shape.flow_count
    ctx = rsv.Context(0)
    batch = _upload(rsv, [read_proof(A)])
    outs = []
    for grouped in (False, True):
        plonk, poseidon, ops = _full((1, 12, 1 << lp), torch.int32), _full((1, 48, 1 << lq), torch.int32), _full((1, n_ops), torch.int32)
        if grouped:
            d_vars, d_acc, _, _, d_flow, d_swap = _eval(rsv, ctx, wp, [("A", "A")])
            ctx.witness_trace_groups(wp, d_vars, d_acc, 1, d_plonk=plonk, d_poseidon=poseidon, d_ops=ops, d_flow=d_flow, d_flow_swap=d_swap)
        else:
            d_vars, d_acc = _full((1, wp.n_vars, 4), torch.int32), _full((1,), torch.uint8)
            d_flow, d_swap = _full((1, F, 32), torch.int32), _full((1, F), torch.uint8)
            ctx.witness(wp, *batch, 1, d_vars, d_acc, inputs=inputs_of(A), d_flow=d_flow, d_flow_swap=d_swap)
            ctx.witness_trace(wp, d_vars, d_acc, 1, d_plonk=plonk, d_poseidon=poseidon, d_ops=ops, d_flow=d_flow, d_flow_swap=d_swap)
        ctx.synchronize()
        assert d_acc.cpu().tolist() == [1]
        outs.append((d_vars, plonk, poseidon, ops))
    for name, x, y in zip(("variables", "plonk", "poseidon", "ops"), *outs):
        assert torch.equal(x, y), name
    assert outs[0][1].min() >= 0  # nothing of the prefill is left (canonical M31 words)
    ctx.close()


def _dev32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64) % (1 << 32), dtype=np.uint32).view(np.int32)).to(DEV)


@pytest.mark.parametrize("n_groups", [1, 3, 70])
def test_launch_forms_agree(rsv, wp, n_groups):
    """n_groups groups whose members alternate A, B (70: a rejected group, [tamper(A), B], at slots 63 and 64), witness and
    trace, under every witness launch form and in both variable layouts.  Under every form: the verdicts and the members'
    reasons; every accepted group's `variables` are the oracle's [A, B] vector, its flow slots the C oracle's flows of A and
    B, and its Plonk, Poseidon and ops columns (witness_trace_groups on that form's outputs) the oracle's columns of the
    single group [A, B]; the rejected groups' columns are zero.  So all forms agree with each other and with the
    single-group values.  70 puts the n >= 64 wide form and a second workgroup of groups in play, for the trace kernels a
    group stride past 64 in both layouts.  Compared on the device; the column buffers are prefilled again before every trace."""
    import torch
    rejected = {63, 64} if n_groups == 70 else set()
    groups = [("bad", "B") if g in rejected else ("A", "B") for g in range(n_groups)]
    proofs = _proofs()
    batch = _upload(rsv, [proofs[k] for g in groups for k in g])
    lp, lq = wp.trace_sizes()
    op_rows = wp.gates()[1][:, 0]
    want_plonk, want_poseidon, want_op = R.columns((A, B), lp, lq)
    want = {"variables": _dev32(R.variables((A, B))), "plonk": _dev32(want_plonk), "poseidon": _dev32(want_poseidon), "ops": _dev32(want_op[op_rows])}
    flows = [ob.poseidon_flow(read_proof(name), inputs_of(A)) for name in (A, B)]
    want_flow = _dev32(np.stack([f[:, :32] for f in flows]))
    want_swap = torch.from_numpy(np.stack([f[:, 32] for f in flows]).astype(np.uint8)).to(DEV)
    good = torch.tensor([g not in rejected for g in range(n_groups)], device=DEV)
    cols = {"plonk": _full((n_groups, 12, 1 << lp), torch.int32), "poseidon": _full((n_groups, 48, 1 << lq), torch.int32),
            "ops": _full((n_groups, len(op_rows)), torch.int32)}
    ctx = rsv.Context(0)
    for by_variable in (False, True):
        ctx.set_option("witness_layout", "by_variable" if by_variable else "by_proof")
        for launch in LAUNCH_FORMS:
            with launch_form(ctx, launch, n_groups):
                d_vars, d_acc, d_macc, d_mreason, d_flow, d_swap = _eval(rsv, ctx, wp, groups, by_variable=by_variable, batch=batch)
            for t in cols.values():
                t.fill_(-1)
            ctx.witness_trace_groups(wp, d_vars, d_acc, n_groups, d_plonk=cols["plonk"], d_poseidon=cols["poseidon"], d_ops=cols["ops"],
                                     d_flow=d_flow, d_flow_swap=d_swap)
            ctx.synchronize()
            form = (by_variable, *launch)
            assert torch.equal(d_acc != 0, good), form
            assert torch.equal(d_macc[:, 0] != 0, good) and bool(d_macc[:, 1].all()), form
            assert torch.equal(d_mreason[:, 0] == 0, good) and not bool(d_mreason[:, 1].any()), form
            assert bool((d_flow[good] == want_flow[None]).all()) and bool((d_swap[good] == want_swap[None]).all()), form
            assert bool((d_flow[~good][:, 1] == want_flow[None, 1]).all()), form  # the verified member of a rejected group
            rows = d_vars.permute(1, 0, 2) if by_variable else d_vars
            assert bool((rows[good] == want["variables"][None]).all()), form
            for name, t in cols.items():
                same = (t == want[name][None]).flatten(1).all(dim=1)
                assert torch.equal(same, good), (form, name)
                assert not bool(t[~good].any()), (form, name)
    ctx.close()


def test_columns_of_mixed_groups(rsv, wp):
    """The trace of [A,B], [B,A] and the rejected [A, tamper(A)]: Plonk [12, 2^17] and Poseidon [48, 2^16] columns and the
    ops, against oracle.recursion_circuit.trace's columns of the oracle's circuit of each group; the rejected group's are zero."""
    import torch
    groups = [("A", "B"), ("B", "A"), ("A", "bad")]
    lp, lq = wp.trace_sizes()
    assert (lp, lq) == (17, 16)
    op_rows = wp.gates()[1][:, 0]
    n, n_ops = len(groups), len(op_rows)
    ctx = rsv.Context(0)
    d_vars, d_acc, _, _, d_flow, d_swap = _eval(rsv, ctx, wp, groups)
    plonk, poseidon, ops = _full((n, 12, 1 << lp), torch.int32), _full((n, 48, 1 << lq), torch.int32), _full((n, n_ops), torch.int32)
    ctx.witness_trace_groups(wp, d_vars, d_acc, n, d_plonk=plonk, d_poseidon=poseidon, d_ops=ops, d_flow=d_flow, d_flow_swap=d_swap)
    ctx.synchronize()
    plonk, poseidon, ops = _u32(plonk), _u32(poseidon), _u32(ops)
    ctx.close()
    seen = []
    for k, g in enumerate(groups[:2]):
        want_plonk, want_poseidon, want_op = R.columns(tuple({"A": A, "B": B}[x] for x in g), lp, lq)
        assert np.array_equal(plonk[k], want_plonk), g
        assert np.array_equal(poseidon[k], want_poseidon), g
        assert np.array_equal(ops[k], want_op[op_rows]), g
        seen.append(want_op[op_rows])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(plonk[0], plonk[1])
    assert not plonk[2].any() and not poseidon[2].any() and not ops[2].any()


def _whole_chain(rsv, ctx, wp, flat, n, inputs, cfg):
    ch = rsv.Chain(ctx, wp, n, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, device=DEV, aggregate=True)
    ch.witness(flat, inputs)
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch, stage)()
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.open()
    ch.fri_open()
    return ch


def test_whole_chain_of_groups(rsv, wp):
    """Chain(aggregate=True) on [[A,B], [A, tamper(A)], [B,A]] at pow_bits 12, b = 1, log_last 8, 10 queries, with the caps:
    one next proof per accepted group, which the C oracle and the library's verifier accept; the rejected group's slot is
    zero / None; the two accepted groups' proofs differ in roots, draws and nonce; pack() gives the bytes of proofs()."""
    cfg = Cfg(12, 1, 8, 10)
    proofs = _proofs()
    flat = [proofs[k] for k in ("A", "B", "A", "bad", "B", "A")]
    ctx = rsv.Context(0)
    ch = _whole_chain(rsv, ctx, wp, flat, 3, inputs_of(A), cfg)
    got, out = ch.numpy(), ch.proofs()
    d_blob, d_off = ch.pack(exact=True)
    blob, off = d_blob.cpu().numpy().tobytes(), d_off.cpu().tolist()
    ctx.close()
    assert got["ok"].tolist() == [1, 0, 1] and got["acc"].tolist() == [1, 0, 1]
    assert got["member_accept"].tolist() == [[1, 1], [1, 0], [1, 1]] and got["member_reason"][1, 1] != 0
    assert out[1] is None and out[0] is not None and out[2] is not None
    assert [key for key in got if not key.startswith("member_") and got[key][1].any()] == []
    for key in ("roots", "draws", "nonce"):
        assert not np.array_equal(got[key][0], got[key][2]), key
    for verify in (ob.verify_batch, rsv.verify_batch):
        acc, reason = verify([out[0], out[2]], cfg, inputs_of(B))
        assert acc.tolist() == [1, 1] and reason.tolist() == [0, 0], (verify.__module__, acc.tolist(), reason.tolist())
    assert off == np.cumsum([0] + [len(p) if p else 0 for p in out]).tolist()
    assert blob == b"".join(p or b"" for p in out)


def test_the_references_own_aggregation(rsv):
    """Five copies of recursive_proof_16_15.bin as ONE group under the 5-copy program of its pair and the pair's
    configuration: the chain puts out level1-5.bin byte for byte, as it does through the existing path
    (tests/test_proof_bytes_gpu.py)."""
    pin = pin_of("recursive_proof_16_15.bin", 5)
    src, dst = pin["src"], pin["dst"]
    assert dst == "level1-5.bin"
    prog = program_of(rsv, pin)
    ctx = rsv.Context(0)
    ch = _whole_chain(rsv, ctx, prog, [read_proof(src)] * 5, 1, inputs_of(src), fixture_cfg(dst))
    out = ch.proofs()
    assert ch.numpy()["member_accept"].tolist() == [[1] * 5]
    ctx.close()
    prog.close()
    want = read_proof(dst)
    assert out[0] is not None and len(out[0]) == len(want) and out[0] == want


def test_misuse(rsv, wp):
    """A created (not built) program, a configuration that is not the program's and n_groups * copies > 2^20 are RSV_E_SIZE;
    d_flow without d_flow_swap is RSV_E_NULL."""
    import torch
    groups = [("A", "B")]
    ctx = rsv.Context(0)
    created = rsv.WitnessProgram(wp.export())
    with pytest.raises(rsv.RsvError) as e:
        _eval(rsv, ctx, created, groups)
    assert e.value.code == -2
    with pytest.raises(rsv.RsvError) as e:
        created.group_scratch_bytes(1)
    assert e.value.code == -2
    created.close()
    other = rsv.WitnessProgram.build(read_proof(A), fixture_cfg(A), inputs_of(A), copies=COPIES, set_walks=R.walks())
    other.shape.n_queries = 9  # what cfg() reports to the call below
    with pytest.raises(rsv.RsvError) as e:
        _eval(rsv, ctx, other, groups)
    assert e.value.code == -2
    other.close()
    batch = _upload(rsv, [read_proof(A), read_proof(B)])
    n, m, F = 1, COPIES, wp.shape.flow_count
    d_vars, d_acc, d_macc = _full((n, wp.n_vars, 4), torch.int32), _full((n,), torch.uint8), _full((n, m), torch.uint8)
    with pytest.raises(rsv.RsvError) as e:  # refused before anything is read: the batch does not have to hold that many proofs
        ctx.witness_groups(wp, *batch, (1 << 20) // COPIES + 1, d_vars, d_acc, d_macc, inputs=inputs_of(A))
    assert e.value.code == -2
    with pytest.raises(rsv.RsvError) as e:
        ctx.witness_groups(wp, *batch, n, d_vars, d_acc, d_macc, inputs=inputs_of(A), d_flow=_full((n, m, F, 32), torch.int32))
    assert e.value.code == -1
    ctx.synchronize()
    assert d_acc.cpu().tolist() == [255]  # nothing was written
    ctx.close()
