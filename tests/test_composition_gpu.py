"""rsv_composition_dev / rsv_witness_tree3_dev (`-m gpu`): tree 3 of the next proof, the composition polynomial.  Against
the REFERENCE for all 14 consecutive fixture pairs (the chain of fixture K gives K+1's commitments[3], the OODS point its
transcript draws behind that root and its sampled_values[3]), bit for bit against the numpy restatement
(tests/composition_ref.py, pinned to the reference by tests/test_composition_host.py) on random canonical columns at the
smallest shapes where a path changes, the coefficients output, a workspace budget that cuts rows and proofs, the largest
words, and the refusals.  Every comparison is exact on 32-bit words and covers every element; outputs are prefilled with
0xffffffff."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import composition_ref as K
from tests import oracle_binding as ob
from tests.chain_harness import DEV, chain, dev, full, inputs_of, mask_dev, masked_past_64, next_samples, pin_id, pins, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = C.P


def _want3(dst):
    from oracle import recursion_circuit as rc
    nxt = read_proof(dst)
    d = rc.parse_proof(nxt)
    tr = ob.transcript_raw(nxt)
    root = np.array([int(x) for x in d.commitments[3]], dtype=np.uint32)
    samples = np.array([v for col in d.sampled_values[3] for v in col], dtype=np.uint32)
    assert samples.shape == (8, 4)
    return root, np.array(tr[20:28], dtype=np.uint32), samples


ROUND_TRIP = "level2-1.bin"  # the one pair whose OODS point is fed back into witness_sample (test_sample_gpu.py pins the rest)


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_chain_gives_what_the_next_fixture_carries(rsv, pin):
    """witness_tree3 of fixture K: K+1's commitments[3], its OODS point (transcript_raw words 20..27) and its
    sampled_values[3]; for one pair, witness_sample fed with the returned d_oods gives K+1's other 134 values."""
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    b = fixture_cfg(dst).log_blowup_factor
    root, oods, samples = _want3(dst)
    ctx = rsv.Context(0)
    ch = chain(rsv, ctx, wp, [read_proof(src)], inputs_of(src), b, upto="tree3")
    got = ch.numpy()
    assert got["ok"].tolist() == [1]
    assert np.array_equal(got["root3"][0], root)
    assert np.array_equal(got["oods"][0], oods)
    assert np.array_equal(got["samples3"][0], samples)
    if src == ROUND_TRIP:
        want, _ = next_samples(dst)
        ch.sample()
        assert np.array_equal(ch.numpy()["samples"][0], want)
    ctx.close()
    wp.close()


def test_batch_with_a_rejected_proof(rsv):
    """Three proofs, the middle one tampered: zeros everywhere for it, the solo values for the other two."""
    pin = next(p for p in pins() if p["src"] == ROUND_TRIP)
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    b = fixture_cfg(dst).log_blowup_factor
    root, oods, samples = _want3(dst)
    proof = read_proof(src)
    ctx = rsv.Context(0)
    solo = chain(rsv, ctx, wp, [proof], inputs_of(src), b, upto="tree3", caps=True).numpy()
    got = chain(rsv, ctx, wp, [proof, ob.tamper(proof, 5), proof], inputs_of(src), b, upto="tree3", caps=True).numpy()
    ctx.close()
    wp.close()
    assert got["ok"].tolist() == [1, 0, 1]
    for k in ("comp", "root3", "oods", "samples3", "cap3", "channel"):
        assert np.array_equal(got[k][0], solo[k][0]) and np.array_equal(got[k][2], solo[k][0]), k
        assert not got[k][1].any(), k
    assert np.array_equal(solo["root3"][0], root) and np.array_equal(solo["oods"][0], oods) and np.array_equal(solo["samples3"][0], samples)
    assert np.array_equal(solo["cap3"][0, 1], root) and not solo["cap3"][0, 0].any()


# ---------------------------------------------------------------- rsv_composition_dev on random columns
def _random_inputs(rng, lp, lq, n, shared, value=None):
    """plonk, poseidon: (preprocessed, trace, interaction) int64[n or 1, cols, 2^log]; sums [n, 2, 4], draws [n, 12]."""
    draw = (lambda shape: rng.integers(0, P, shape)) if value is None else (lambda shape: np.full(shape, value, np.int64))
    plonk = [draw((1 if shared else n, 10, 1 << lp)), draw((n, 12, 1 << lp)), draw((n, 8, 1 << lp))]
    poseidon = [draw((1 if shared else n, 40, 1 << lq)), draw((n, 48, 1 << lq)), draw((n, 8, 1 << lq))]
    return plonk, poseidon, draw((n, 2, 4)), draw((n, 12))


def _run(rsv, ctx, lp, lq, plonk, poseidon, sums, draws, n, mask=None, coeffs=True, shared=False):
    L3 = rsv.composition_log_size(lp, lq)
    d_comp = full((n, 8, 1 << L3))
    d_co = full((n, 8, 1 << L3)) if coeffs else None
    d_mask = mask_dev(mask)
    dp, dq = [dev(c) for c in plonk], [dev(c) for c in poseidon]
    if shared:
        dp[0], dq[0] = dp[0][0], dq[0][0]  # [cols, 2^log]: proof stride 0
    d_sums, d_draws = dev(sums), dev(draws)
    ctx.composition(lp, lq, dp, dq, d_sums, d_draws, n, d_comp, d_co, d_mask=d_mask)
    ctx.synchronize()
    return u32(d_comp), (u32(d_co) if coeffs else None), (d_comp, d_co)


def _ref(plonk, poseidon, lp, lq, sums, draws, p):
    mine = lambda cols: [c[0 if c.shape[0] == 1 else p] for c in cols]  # noqa: E731
    return K.composition(mine(plonk), mine(poseidon), lp, lq, sums[p], draws[p])


SHAPES = K.SHAPES


def _check_shape(rsv, lp, lq, n, mask, shared, seed):
    """Random canonical columns, sums and draws: d_comp and d_comp_coeffs equal the restatement's, d_comp_coeffs is
    C.interpolate of d_comp, the run without d_comp_coeffs gives the same columns, a masked proof is zero."""
    rng = np.random.default_rng(seed)
    plonk, poseidon, sums, draws = _random_inputs(rng, lp, lq, n, shared)
    ctx = rsv.Context(0)
    comp, co, _ = _run(rsv, ctx, lp, lq, plonk, poseidon, sums, draws, n, mask, True, shared)
    alone, _, _ = _run(rsv, ctx, lp, lq, plonk, poseidon, sums, draws, n, mask, False, shared)
    ctx.close()
    assert np.array_equal(alone, comp)
    L3 = rsv.composition_log_size(lp, lq)
    assert np.array_equal(co, C.interpolate(comp.astype(np.int64), L3))
    for p in range(n):
        if mask is not None and not mask[p]:
            assert not comp[p].any() and not co[p].any(), p
            continue
        want, want_co = _ref(plonk, poseidon, lp, lq, sums, draws, p)
        assert np.array_equal(co[p], want_co), (seed, p)
        assert np.array_equal(comp[p], want), (seed, p)


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=lambda k: "lp%d_lq%d" % SHAPES[k][:2])
def test_composition_bit_for_bit(rsv, case):
    """SHAPES through _check_shape: d_comp and d_comp_coeffs equal the restatement's, a masked proof is zero."""
    lp, lq, n, mask, shared = SHAPES[case]
    _check_shape(rsv, lp, lq, n, mask, shared, 1700 + case)


def test_composition_past_one_workgroup_of_proofs(rsv):
    """(lp, lq) = (4, 3), 70 proofs, 63 and 64 masked: k_co_params' second workgroup of proofs, every proof against the
    restatement."""
    _check_shape(rsv, 4, 3, 70, masked_past_64(), False, 1730)


def test_coefficients_sample_as_the_columns(rsv):
    """sample_tree(source=COEFFS) on d_comp_coeffs equals sample_tree on d_comp, at two points per proof."""
    lp, lq, n = 5, 4, 2
    rng = np.random.default_rng(1710)
    plonk, poseidon, sums, draws = _random_inputs(rng, lp, lq, n, False)
    ctx = rsv.Context(0)
    _, _, (d_comp, d_co) = _run(rsv, ctx, lp, lq, plonk, poseidon, sums, draws, n)
    L3 = rsv.composition_log_size(lp, lq)
    pts = dev(rng.integers(0, P, (n, 2, 8)))
    a, c = full((n, 2, 8, 4)), full((n, 2, 8, 4))
    ctx.sample_tree([{"log_size": L3, "d_cols": d_comp, "n_cols": 8}], n, pts, 2, a, source=rsv.SAMPLE_COLUMNS)
    ctx.sample_tree([{"log_size": L3, "d_cols": d_co, "n_cols": 8}], n, pts, 2, c, source=rsv.SAMPLE_COEFFS)
    ctx.synchronize()
    ctx.close()
    assert np.array_equal(u32(a), u32(c)) and u32(a).any() and not (u32(a) == 0xFFFFFFFF).any()


def _pass_size(lp, lq, n, shared, budget, coeffs):
    """The driver's pass restated (composition_api.inc: co_ws_bytes and the two halving loops) -> (proofs per pass, blocks
    of 2^(max(lp, lq) + 1) rows per pass, bytes of the whole batch uncut).  Per group the coefficients and the extended rows
    in flight (one set for a shared group), 92 x 4 parameter words per proof, the two 1/Z tables, the accumulator (4 x 2^clb
    per proof) and, without d_comp_coeffs, the cut coefficients; every part on a 256-byte boundary."""
    clb = K.clb_of(lp, lq)
    groups = [(lp, 10, shared), (lp, 12, False), (lp, 8, False), (lq, 40, shared), (lq, 48, False), (lq, 8, False)]

    def ws(m, nc):
        rows = nc << (max(lp, lq) + 1)
        parts = []
        for log, cols, sh in groups:
            parts += [((1 if sh else m) * cols) << log, (1 if sh else m) * cols * rows]
        parts += [m * 92 * 4, 1 << (clb - lp), 1 << (clb - lq), (m * 4) << clb] + ([] if coeffs else [(m * 4) << clb])
        off = 0
        for words in parts:
            off = ((off + 255) & ~255) + 4 * words
        return off
    m, nc = n, 1 << (clb - max(lp, lq) - 1)
    whole = ws(m, nc)
    while ws(m, nc) > budget and nc > 1:
        nc >>= 1
    while ws(m, nc) > budget and m > 1:
        m = (m + 1) // 2
    return m, nc, whole


def test_composition_under_a_small_workspace_budget(rsv):
    """19 proofs of (lp, lq) = (6, 6), shared preprocessed columns, three proofs masked.  The whole batch needs 3 626 496
    bytes in one pass of all four blocks of 128 rows; under a 1 MB budget the driver first streams one block at a time
    (1 331 712 bytes, still too many), then halves the proofs to 10 a pass (719 360 bytes; passes of 10 + 9): both cuts
    happen, the previous-row neighbours cross from one 64-row half of a block to the other, and the caller's buffers are
    read at p0 = 10.  _pass_size restates the driver's arithmetic and the test asserts the figures, so it cannot go vacuous
    if the layout changes.  Every element of the cut run equals the uncut run, and the uncut run the restatement."""
    lp, lq, n = 6, 6, 19
    budget = 1 << 20
    assert _pass_size(lp, lq, n, True, budget, True) == (10, 1, 3626496)
    assert _pass_size(lp, lq, n, True, 1331712, True)[:2] == (n, 1) and _pass_size(lp, lq, 10, True, 719360, True)[:2] == (10, 1)
    assert _pass_size(lp, lq, n, True, 8192 << 20, True)[:2] == (n, 4)
    rng = np.random.default_rng(1720)
    plonk, poseidon, sums, draws = _random_inputs(rng, lp, lq, n, True)
    mask = [0 if p in (0, 9, 18) else 1 for p in range(n)]
    ctx = rsv.Context(0)
    whole, whole_co, _ = _run(rsv, ctx, lp, lq, plonk, poseidon, sums, draws, n, mask, True, True)
    ctx.set_option("ws_budget_mb", 1)
    cut, cut_co, _ = _run(rsv, ctx, lp, lq, plonk, poseidon, sums, draws, n, mask, True, True)
    ctx.close()
    assert np.array_equal(cut, whole) and np.array_equal(cut_co, whole_co)
    for p in range(n):
        if not mask[p]:
            assert not whole[p].any() and not whole_co[p].any(), p
            continue
        want, want_co = _ref(plonk, poseidon, lp, lq, sums, draws, p)
        assert np.array_equal(whole[p], want) and np.array_equal(whole_co[p], want_co), p


def test_largest_words(rsv):
    """Every input column, sum and draw word at P - 1, the largest canonical word, equals the restatement.  What this
    reaches: the largest operands of every m_* and q_* step of the row kernels and the largest powers' words the draws
    allow.  What it does not: the edge of the unreduced u64 sums.  Their operands are a constraint value and a word of a
    power of random_coeff, both results of modular arithmetic on the inputs and not under the test's control, so the sums
    stay far from 4 (2^31 - 2)^2 + 2^34; the bound next to CoAcc covers any canonical operands."""
    lp, lq = 4, 3
    plonk, poseidon, sums, draws = _random_inputs(None, lp, lq, 1, False, value=P - 1)
    ctx = rsv.Context(0)
    comp, co, _ = _run(rsv, ctx, lp, lq, plonk, poseidon, sums, draws, 1)
    ctx.close()
    want, want_co = _ref(plonk, poseidon, lp, lq, sums, draws, 0)
    assert np.array_equal(comp[0], want) and np.array_equal(co[0], want_co)


def test_device_refusals(rsv):
    """NULL pointers, sizes and misalignment with a live context: the neighbours' codes, nothing written."""
    import torch
    dev = torch.device(DEV)
    lp, lq, n = 4, 3, 1
    ctx = rsv.Context(0)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    plonk, poseidon = [z(1, 10, 16), z(1, 12, 16), z(1, 8, 16)], [z(1, 40, 8), z(1, 48, 8), z(1, 8, 8)]
    sums, draws = z(1, 2, 4), z(1, 12)
    raw = torch.zeros(8192, dtype=torch.uint8, device=dev)
    out = torch.full((1, 8, 32), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    co = torch.full((1, 8, 32), 0x5A5A5A5A, dtype=torch.int32, device=dev)

    def refused(code, lp=lp, lq=lq, plonk=plonk, poseidon=poseidon, sums=sums, draws=draws, n=n, d_comp=out, d_co=co):
        with pytest.raises(rsv.RsvError) as e:
            ctx.composition(lp, lq, plonk, poseidon, sums, draws, n, d_comp, d_co)
        assert e.value.code == code, (code, e.value.code)

    for k in range(3):
        refused(-1, plonk=[None if i == k else t for i, t in enumerate(plonk)])
        refused(-1, poseidon=[None if i == k else t for i, t in enumerate(poseidon)])
    refused(-1, sums=None)
    refused(-1, draws=None)
    refused(-1, d_comp=None)
    refused(-2, lp=1)
    refused(-2, lq=1)
    refused(-2, lp=29)
    refused(-2, lq=28)
    refused(-2, n=(1 << 20) + 1)
    refused(-2, sums=raw[1:33])
    refused(-2, draws=raw[2:50])
    refused(-2, d_comp=raw[1:1025])
    refused(-2, d_co=raw[2:1026])
    refused(-2, plonk=[plonk[0], raw[1:769], plonk[2]])
    ctx.synchronize()
    assert bool((out == 0x5A5A5A5A).all()) and bool((co == 0x5A5A5A5A).all())
    ctx.composition(lp, lq, plonk, poseidon, sums, draws, n, out, co)
    ctx.synchronize()
    assert not bool(out.any()) and not bool(co.any())  # zero columns: every constraint is zero, every word written
    ctx.close()
