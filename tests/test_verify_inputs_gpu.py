"""A batch in which every proof has its own public inputs (`-m gpu`): rsv_public_input_sum_dev, rsv_verify_batch_inputs_dev,
rsv_verify_hints_inputs_dev, rsv_verify_batch_inputs, rsv_circuit_inputs_dev, Chain.inputs and Chain.verify.  Everything is
exact on 32-bit words and verdict bytes.

1 and 2 run the kernel alone against the Python-integer model of tests/verify_inputs_ref.py (which
tests/test_verify_inputs_host.py ties to the oracle's field operations): the sizes at which a lane gets its first term, a
wave its second round (64 -> 65), a lane its second chunk (4 096 inputs: eight chunks), batches that end inside a workgroup of
four proofs; then crafted rows.  3 gives the per-proof call every fixture's shared inputs replicated and wants the shared
call's bytes.  4-6 verify what the chain proves with the statements the chain holds, against the C oracle called per proof."""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import user_circuit_ref as U
from tests import verify_inputs_ref as V
from tests.chain_harness import DEV, FILL, chain, inputs_of, pin_of, program_of, u32
from tests.conftest import fixture_cfg, load_manifest, read_proof

pytestmark = pytest.mark.gpu
P = V.P
R_PARSE, R_LOGUP = 1, 3
CONFIG = (3, 1, 0, 9)          # (pow_bits, log_blowup, log_last, n_queries): tests/test_user_circuit_gpu.py's first


@pytest.fixture(scope="module")
def ctx(rsv):
    c = rsv.Context(0)
    yield c
    c.close()


def _dev(a, dtype=np.uint32):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).to(DEV)


# ---------------------------------------------------------------- 1. the kernel alone, random terms
def _sum(ctx, rec, za, with_bad=True):
    """rec uint32[n, n_pi, 5], za uint32[n, 8] -> (sum uint32[n, 4], bad uint8[n]); outputs prefilled."""
    import torch
    n, n_pi = rec.shape[:2]
    d_sum = torch.full((n, 4), -1, dtype=torch.int32, device=DEV)
    d_bad = torch.full((n,), 7, dtype=torch.uint8, device=DEV) if with_bad else None
    ctx.public_input_sum(_dev(rec) if n_pi else None, n, n_pi, _dev(za), d_sum, d_bad)
    ctx.synchronize()
    return u32(d_sum), (d_bad.cpu().numpy() if with_bad else None)


def _random_batch(rnd, n, n_pi):
    rec = np.zeros((n, n_pi, 5), np.uint32)
    rec[:, :, 0] = rnd.integers(0, 1 << 32, (n, n_pi), dtype=np.uint64)      # any u32, P and beyond included: taken mod P
    rec[:, :, 1:] = rnd.integers(0, P, (n, n_pi, 4))
    return rec, rnd.integers(0, P, (n, 8)).astype(np.uint32)


@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("n_pi", [0, 1, 15, 16, 17, 63, 64, 65, 129, 4096])
def test_kernel_alone_random_terms(rsv, ctx, n, n_pi):
    rnd = np.random.default_rng(1000 * n + n_pi)
    rec, za = _random_batch(rnd, n, n_pi)
    if n_pi:
        rec[0, 0, 0] = P + 5                                                 # idx >= P
    got, bad = _sum(ctx, rec, za)
    want = [V.model(rec[p], za[p, :4], za[p, 4:]) for p in range(n)]
    assert bad.tolist() == [0] * n
    assert got.tolist() == [w[0] for w in want]
    if n_pi == 0:
        assert not got.any()
    if n == 3:                                                               # d_bad is optional
        assert np.array_equal(_sum(ctx, rec, za, with_bad=False)[0], got)


# ---------------------------------------------------------------- 2. crafted rows
def test_kernel_alone_crafted_rows(rsv, ctx):
    """n_pi = 129: lane 0 holds terms 0, 64 and 128 in one chunk, lane 1 terms 1 and 65.  Proof by proof: a zero denominator
    alone; two in lane 0's chunk; one in every lane; all three of lane 0 (the chunk's product is empty); idx >= P on a zero
    term; a value word = P; a value word = 0xffffffff; both in one record; a word of z = P.  Between them untouched random
    proofs whose sums must be their own."""
    rnd = np.random.default_rng(5)
    n_pi = 129
    rec, za = _random_batch(rnd, 14, n_pi)

    def zero(p, k, idx=None):
        if idx is not None:
            rec[p, k, 0] = idx
        rec[p, k, 1:] = V.value_for_zero(rec[p, k, 0], za[p, :4], za[p, 4:])
    zero(1, 70)
    zero(2, 0), zero(2, 64)
    for k in range(64):
        zero(4, k + 64 * (k % 2))
    zero(5, 0), zero(5, 64), zero(5, 128)
    zero(7, 128, idx=P + 9), zero(7, 3, idx=0xFFFFFFFF)
    rec[8, 77, 2] = P
    rec[10, 128, 4] = 0xFFFFFFFF
    rec[11, 0, 1], rec[11, 0, 3] = 0xFFFFFFFF, P
    za[12, 1] = P
    want_bad = [1 if p in (8, 10, 11, 12) else 0 for p in range(14)]
    got, bad = _sum(ctx, rec, za)
    want = [V.model(rec[p], za[p, :4], za[p, 4:]) for p in range(14)]
    assert [w[1] for w in want] == want_bad and bad.tolist() == want_bad
    assert got.tolist() == [w[0] for w in want]
    for p, zeros in ((1, 1), (2, 2), (4, 64), (5, 3), (7, 2)):
        assert sum(d == V.ZERO for d in V.denominators(rec[p], za[p, :4], za[p, 4:])[0]) == zeros
    # the offending word counts as 0: the same proofs with the word cleared, none of them bad, the same sums
    clean, za_clean = rec.copy(), za.copy()
    clean[:, :, 1:][clean[:, :, 1:] >= P] = 0
    za_clean[za_clean >= P] = 0
    got_clean, bad_clean = _sum(ctx, clean, za_clean)
    assert np.array_equal(got_clean, got) and not bad_clean.any()
    # a proof's sum does not depend on its neighbours: every proof alone
    for p in (0, 1, 5, 8, 9, 13):
        solo, solo_bad = _sum(ctx, rec[p:p + 1], za[p:p + 1])
        assert solo[0].tolist() == want[p][0] and solo_bad.tolist() == [want_bad[p]]


# ---------------------------------------------------------------- 3. shared against per-proof
REJECTS = ["small_proof_composition.bin", "small_proof_dup_query.bin", "recursive_proof_16_15_composition.bin", "level1-5_dup_query.bin"]


def _fixture_batch():
    names = [e["file"] for e in load_manifest()] + REJECTS
    proofs = [read_proof(nm) for nm in names]
    cfgs = [fixture_cfg(nm) for nm in names]
    return names, proofs, cfgs


def _verify_dev(rsv, ctx, proofs, cfgs, inputs=None, own=None):
    import torch
    blob, offsets = rsv.pack(proofs)
    n = len(proofs)
    d_blob, d_off = torch.from_numpy(blob.copy()).to(DEV), torch.from_numpy(offsets.astype(np.int64)).to(DEV)
    d_acc, d_reason = torch.full((n,), 7, dtype=torch.uint8, device=DEV), torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    if own is None:
        ctx.verify_batch(d_blob, d_off, n, d_acc, d_reason, cfg=cfgs, inputs=inputs)
    else:
        ctx.verify_batch(d_blob, d_off, n, d_acc, d_reason, cfg=cfgs, d_inputs=_dev(own), n_inputs=own.shape[1])
    ctx.synchronize()
    return d_acc.cpu().numpy(), d_reason.cpu().numpy()


@pytest.mark.parametrize("form", ["row", "lane"])
def test_replicated_inputs_give_the_shared_calls_bytes(rsv, ctx, form):
    """Every fixture of the manifest (the Poseidon-channel ones, the two of other formats) and the re-ground reject fixtures
    under their own configurations (cfg_of), at 21 proofs (a partly filled workgroup of every kernel) and, with the small
    ones repeated and tampered, at 70 (past one 64-lane workgroup of the lane form).  The shared inputs are the standard three
    (what every fixture but small_proof.bin is verified under) and small_proof.bin's one: a fixture verified under the other
    set is rejected by both calls alike."""
    names, proofs, cfgs = _fixture_batch()
    small = read_proof("small_proof.bin")
    many = proofs + [ob.tamper(small, i) if i % 3 == 2 else small for i in range(70 - len(proofs))]
    many_cfgs = cfgs + [fixture_cfg("small_proof.bin")] * (70 - len(proofs))
    ctx.set_option("oods_form", form)
    try:
        for batch, bc in ((proofs, cfgs), (many, many_cfgs)):
            n = len(batch)
            assert n % 4 and n % 16 and n % 64
            for shared in (rsv.STANDARD_INPUTS, inputs_of("small_proof.bin")):
                want = _verify_dev(rsv, ctx, batch, bc, inputs=shared)
                got = _verify_dev(rsv, ctx, batch, bc, own=np.stack([V.records_of(shared)] * n))
                assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist(), (form, n, len(shared))
                accepted = {nm for nm, a in zip(names, want[0]) if a}
                if len(shared) == 3:
                    assert accepted == {e["file"] for e in load_manifest() if e["expect"] == "ok"} - {"small_proof.bin"}
                else:
                    assert accepted == {"small_proof.bin"}
                    assert want[0][len(names):].tolist() == [0 if i % 3 == 2 else 1 for i in range(n - len(names))]
        # one proof's inputs changed: that proof alone is rejected (the logup balance), its neighbours keep their verdicts
        own = np.stack([V.records_of(rsv.STANDARD_INPUTS)] * len(proofs))
        k = names.index("level3-1.bin")
        own[k, 2, 1] ^= 1
        want = _verify_dev(rsv, ctx, proofs, cfgs, inputs=rsv.STANDARD_INPUTS)
        got = _verify_dev(rsv, ctx, proofs, cfgs, own=own)
        assert (int(got[0][k]), int(got[1][k])) == (0, R_LOGUP) and int(want[0][k]) == 1
        assert np.delete(got[0], k).tolist() == np.delete(want[0], k).tolist() and np.delete(got[1], k).tolist() == np.delete(want[1], k).tolist()
    finally:
        ctx.set_option("oods_form", "auto")


def test_hints_call_with_a_flow_output(rsv, ctx):
    """rsv_verify_hints_inputs_dev with the PoseidonFlow as an output: verdicts, flow, swap bytes and counts are the shared
    call's."""
    import torch
    small = read_proof("small_proof.bin")
    cfg, shared = fixture_cfg("small_proof.bin"), inputs_of("small_proof.bin")
    batch = [small, ob.tamper(small, 3), small]
    stride = rsv.poseidon_flow_count(4, 8, cfg)
    blob, offsets = rsv.pack(batch)
    d_blob, d_off = torch.from_numpy(blob.copy()).to(DEV), torch.from_numpy(offsets.astype(np.int64)).to(DEV)
    out = []
    for own in (None, np.stack([V.records_of(shared)] * 3)):
        d_acc, d_reason = torch.full((3,), 7, dtype=torch.uint8, device=DEV), torch.full((3,), 7, dtype=torch.uint8, device=DEV)
        d_flow = torch.zeros((3, stride, 32), dtype=torch.int32, device=DEV)
        d_swap = torch.zeros((3, stride), dtype=torch.uint8, device=DEV)
        d_count = torch.full((3,), -1, dtype=torch.int32, device=DEV)
        kw = {} if own is None else {"d_inputs": _dev(own), "n_inputs": own.shape[1]}
        ctx.verify_hints(d_blob, d_off, 3, d_acc, d_reason, cfg=cfg, inputs=shared, d_flow=d_flow, d_flow_swap=d_swap, d_flow_count=d_count, **kw)
        ctx.synchronize()
        out.append((d_acc.cpu().numpy(), d_reason.cpu().numpy(), u32(d_flow), d_swap.cpu().numpy(), u32(d_count)))
    assert out[0][0].tolist() == [1, 0, 1] and int(out[0][4][0]) == stride
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 4. the chain's own statements
def _finish(ch, cfg):
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch, stage)()
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.open()
    ch.fri_open()
    return ch


def _chain_of(rsv, ctx, circ, builts, by_variable=False):
    cfg = rsv.PcsConfig(*CONFIG)
    ch = rsv.Chain(ctx, circ, len(builts), cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, device=DEV)
    variables = np.stack([b.variables for b in builts])
    ch.load(np.ascontiguousarray(variables.transpose(1, 0, 2)) if by_variable else variables, np.stack([b.unbound_flow() for b in builts]),
            by_variable=by_variable)
    return ch, cfg


def _oracle_each(proofs, cfg, inputs_per_proof):
    acc, reason = zip(*[ob.verify_batch([p], cfg, i) for p, i in zip(proofs, inputs_per_proof)])
    return [int(a[0]) for a in acc], [int(r[0]) for r in reason]


def _verdicts(ctx, pair):
    ctx.synchronize()
    return pair[0].cpu().tolist(), pair[1].cpu().tolist()


@pytest.mark.parametrize("layout", ["by_proof", "by_variable"])
def test_own_statements(rsv, ctx, layout):
    """Three witnesses of S1 that differ in the public input: the chain's statements are each witness's own, one call
    verifies the batch in HBM, the host form agrees with the C oracle called per proof; rotated by one slot every proof is
    rejected as the oracle rejects it; a word = P in one slot's statement is that slot's RSV_R_PARSE."""
    builts = [U.build("S1", pub=(11 + 7 * k, 0, 0, 0), seed=1 + k, bit=k % 2) for k in range(3)]
    circ = rsv.Circuit(builts[0].gates, builts[0].flow_wires, builts[0].n_vars, builts[0].num_input, builts[0].witness_ops)
    ctx.set_option("witness_layout", layout)
    try:
        ch, cfg = _chain_of(rsv, ctx, circ, builts, by_variable=layout == "by_variable")
        ctx.synchronize()
        statements = u32(ch.inputs())
        assert statements.shape == (3, 4, 5)
        assert all(np.array_equal(statements[k], V.records_of(b.inputs)) for k, b in enumerate(builts))
        _finish(ch, cfg)
        assert ch.inputs() is not None and ch._vars is None                 # the statements outlive the variables
        assert _verdicts(ctx, ch.verify(cfg)) == ([1, 1, 1], [0, 0, 0])
        assert _verdicts(ctx, ch.verify(cfg)) == ([1, 1, 1], [0, 0, 0])     # again, on the pair packed before
        proofs = ch.proofs()
        own = [b.inputs for b in builts]
        acc, reason = rsv.verify_batch(proofs, cfg, inputs_per_proof=own)
        assert (acc.tolist(), reason.tolist()) == ([1, 1, 1], [0, 0, 0]) == _oracle_each(proofs, cfg, own)
        rotated = own[1:] + own[:1]
        acc, reason = rsv.verify_batch(proofs, cfg, inputs_per_proof=rotated)
        want = _oracle_each(proofs, cfg, rotated)
        assert want[0] == [0, 0, 0] and (acc.tolist(), reason.tolist()) == want
        got = _verify_dev(rsv, ctx, proofs, cfg, own=np.stack([V.records_of(i) for i in rotated]))
        assert (got[0].tolist(), got[1].tolist()) == want
        # a non-canonical word in slot 1's statement: data, not a refusal; that slot alone
        rec = np.stack([V.records_of(i) for i in own])
        rec[1, 0, 3] = P
        got = _verify_dev(rsv, ctx, proofs, cfg, own=rec)
        assert (got[0].tolist(), got[1].tolist()) == ([1, 0, 1], [0, R_PARSE, 0])
    finally:
        ctx.set_option("witness_layout", "by_proof")
        circ.close()


# ---------------------------------------------------------------- 5. a circuit with many inputs
def test_a_circuit_with_70_public_inputs(rsv, ctx):
    """70 records per proof: past one stride of the wave.  Two witnesses with different statements through the chain, verified
    as a batch with their own statements, swapped (rejected), and against the C oracle per proof."""
    builts = [V.build_many(70, first=11, seed=1), V.build_many(70, first=9000, seed=2, bit=0)]
    circ = rsv.Circuit(builts[0].gates, builts[0].flow_wires, builts[0].n_vars, 70, builts[0].witness_ops)
    try:
        ch, cfg = _chain_of(rsv, ctx, circ, builts)
        _finish(ch, cfg)
        a = ch.numpy()
        assert a["acc"].tolist() == [1, 1] and a["ok"].tolist() == [1, 1]
        statements = u32(ch.inputs())
        assert statements.shape == (2, 70, 5) and all(np.array_equal(statements[k], V.records_of(b.inputs)) for k, b in enumerate(builts))
        assert _verdicts(ctx, ch.verify(cfg)) == ([1, 1], [0, 0])
        proofs, own = ch.proofs(), [b.inputs for b in builts]
        assert _oracle_each(proofs, cfg, own) == ([1, 1], [0, 0])
        swapped = own[::-1]
        acc, reason = rsv.verify_batch(proofs, cfg, inputs_per_proof=swapped)
        want = _oracle_each(proofs, cfg, swapped)
        assert want[0] == [0, 0] and (acc.tolist(), reason.tolist()) == want
    finally:
        circ.close()


# ---------------------------------------------------------------- 6. a built program
def test_a_built_programs_statements_are_the_standard_inputs(rsv, ctx):
    """The smallest fixture pair (small_proof.bin -> recursive_proof_16_15.bin): the recursion circuit has no public input of
    its own, so the chain's statements are the constants 1, i, j — the three standard inputs — and Chain.verify accepts."""
    src = "small_proof.bin"
    pin = pin_of(src)
    cfg = fixture_cfg(pin["dst"])
    wp = program_of(rsv, pin)
    try:
        ch = chain(rsv, ctx, wp, [read_proof(src)] * 2, inputs_of(src), cfg.log_blowup_factor, upto="witness", caps=True,
                   log_last=cfg.log_last_layer_degree_bound)
        _finish(ch, cfg)
        ctx.synchronize()
        statements = u32(ch.inputs())
        assert statements.shape == (2, 3, 5) and all(np.array_equal(s, V.records_of(rsv.STANDARD_INPUTS)) for s in statements)
        assert _verdicts(ctx, ch.verify(cfg)) == ([1, 1], [0, 0])
        assert ch.proofs()[0] == read_proof(pin["dst"])
    finally:
        wp.close()
