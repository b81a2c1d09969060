"""rsv_sample_tree_dev / rsv_witness_sample_dev (`-m gpu`): the sampled values of trees 0, 1 and 2 of the next proof.
Against the REFERENCE for all 14 consecutive fixture pairs (the chain of fixture K sampled at K+1's OODS point gives K+1's
sampled_values[0..2], all 134 values, with nothing else taken from K+1 but log_blowup_factor for the commitment that
precedes), bit for bit against the numpy restatement (tests/sample_ref.py, pinned to the fixtures and to eval_at_point by
tests/test_sample_host.py) on random trees from both sources, at the sizes where the driver and the kernel change path
(2^8 rows: every lane busy; 2^10: the unrolled loop; 2^13 = SP_CHUNK_LOG: more than one chunk per column), with the
unreduced sums at their largest, against the commitment's own LDE at a domain point, and the refusals.  Every comparison
is exact on 32-bit words and covers every element."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import oracle_binding as ob
from tests import sample_ref as S
from tests.chain_harness import CASES, DEV, chain, dev, full, inputs_of, mask_dev, next_samples, pin_id, pins, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = C.P


def _groups_dev(groups, shared=()):
    gs = []
    for i, (log, cols) in enumerate(groups):
        cols = np.ascontiguousarray(np.asarray(cols, dtype=np.int64) % P, dtype=np.uint32)
        if cols.ndim == 2:
            cols = cols[None]
        nc = cols.shape[1]
        gs.append({"log_size": log, "d_cols": dev(cols), "n_cols": nc, "proof_stride": 0 if i in shared else nc << log})
    return gs


def _sample_dev(ctx, gs, n, points, mask=None, source=0):
    """Context.sample_tree on device groups, points uint32[n, k, 8] -> uint32[n, k, sum n_cols, 4]."""
    k = points.shape[1]
    d_out = full((n, k, sum(g["n_cols"] for g in gs), 4))
    d_points, d_mask = dev(points), mask_dev(mask)
    ctx.sample_tree(gs, n, d_points, k, d_out, d_mask=d_mask, source=source)
    ctx.synchronize()
    return u32(d_out)


def _coeffs_dev(ctx, gs, n, b, mask):
    """The groups with d_cols = the d_coeffs of a commit_tree of the same groups (proof_stride: every proof its own)."""
    with_cf = [dict(g, d_coeffs=full((n, g["n_cols"], 1 << g["log_size"]))) for g in gs]
    d_roots, d_mask = full((n, 8)), mask_dev(mask)
    ctx.commit_tree(with_cf, n, b, d_roots, d_mask)
    ctx.synchronize()
    return [{"log_size": g["log_size"], "d_cols": g["d_coeffs"], "n_cols": g["n_cols"]} for g in with_cf]


def _points(rng, n, k):
    return rng.integers(0, P, (n, k, 8)).astype(np.uint32)


def _pt(words8):
    return tuple(int(v) for v in words8[:4]), tuple(int(v) for v in words8[4:])


def _check_random(ctx, spec, b, n, mask, seed, ks=(1, 2, 4)):
    """One random tree: from the evaluations and from a commitment's coefficients, with 1, 2 and 4 points per proof
    (different per proof), every element equals the restatement's; a masked proof is zero."""
    rng = np.random.default_rng(seed)
    groups = [(log, rng.integers(0, P, (1 if sh else n, nc, 1 << log))) for log, nc, sh in spec]
    shared = {i for i, (_, _, sh) in enumerate(spec) if sh}
    gs = _groups_dev(groups, shared)
    gc = _coeffs_dev(ctx, gs, n, b, mask)
    for k in ks:
        pts = _points(rng, n, k)
        from_cols = _sample_dev(ctx, gs, n, pts, mask, 0)
        from_coeffs = _sample_dev(ctx, gc, n, pts, mask, 1)
        assert np.array_equal(from_cols, from_coeffs), (spec, k)
        for p in range(n):
            if mask is not None and not mask[p]:
                assert not from_cols[p].any(), (spec, k, p)
                continue
            mine = [(log, cols[0 if i in shared else p]) for i, (log, cols) in enumerate(groups)]
            want = S.sample_tree(mine, [_pt(pts[p, j]) for j in range(k)])
            assert np.array_equal(from_cols[p], want), (spec, k, p)


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_chain_samples_what_the_next_fixture_carries(rsv, pin):
    """The chain of fixture K at K+1's OODS point: K+1's sampled_values[0..2], all 134 values."""
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    b = fixture_cfg(dst).log_blowup_factor
    want, oods = next_samples(dst)
    ctx = rsv.Context(0)
    ch = chain(rsv, ctx, wp, [read_proof(src)], inputs_of(src), b)
    d_oods = dev(oods[None])
    ch.sample(d_oods)
    r = ch.numpy()
    got = r["samples"]
    ctx.close()
    assert r["ok"].tolist() == [1]
    assert np.array_equal(got[0], want), np.nonzero((got[0] != want).any(axis=1))[0].tolist()
    wp.close()


def test_sample_tree_per_tree_equals_the_chain(rsv):
    """One pair through rsv_sample_tree_dev tree by tree, from the columns and from a commitment's coefficients, at the
    OODS point and the two previous-row points: every value the chain places is there, and a batch with a rejected proof
    gives zeros for it and the solo values for the others."""
    from tests import interaction_ref as R
    pin = next(p for p in pins() if p["src"] == "level2-1.bin")
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    lp, lq = wp.trace_sizes()
    b = fixture_cfg(dst).log_blowup_factor
    want, oods = next_samples(dst)
    proof = read_proof(src)
    ctx = rsv.Context(0)
    ch = chain(rsv, ctx, wp, [proof, ob.tamper(proof, 5), proof], inputs_of(src), b)
    d_oods = dev(np.stack([oods] * 3))
    ch.sample(d_oods)
    r = ch.numpy()
    got = r["samples"]
    assert r["ok"].tolist() == [1, 0, 1]
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want) and not got[1].any()
    ppre, qpre = wp.preprocessed()
    _, wops = wp.gates()
    ppre = ppre.copy()
    if len(wops):
        ppre[3, wops[:, 0]] = r["ops"][0]
    trees = [[(lp, ppre), (lq, qpre)], [(lp, r["plonk"][0]), (lq, r["poseidon"][0])], [(lp, r["int_plonk"][0]), (lq, r["int_poseidon"][0])]]
    o = _pt(oods)
    pts = np.array([[list(q[0]) + list(q[1]) for q in (o, R.prev_row_point(o, lp), R.prev_row_point(o, lq))]], dtype=np.uint32)
    off = 0
    for k, groups in enumerate(trees):
        gs = _groups_dev(groups)
        a = _sample_dev(ctx, gs, 1, pts, None, 0)[0]
        c = _sample_dev(ctx, _coeffs_dev(ctx, gs, 1, b, None), 1, pts, None, 1)[0]
        assert np.array_equal(a, c), k
        col = 0
        for gi, (log, cols) in enumerate(groups):
            for j in range(len(cols)):
                if k == 2 and j >= 4:
                    assert np.array_equal(a[1 + gi, col], want[off]) and np.array_equal(a[0, col], want[off + 1]), (k, gi, j)
                    off += 2
                else:
                    assert np.array_equal(a[0, col], want[off]), (k, gi, j)
                    off += 1
                col += 1
    assert off == 134
    ctx.close()
    wp.close()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_sample_tree_bit_for_bit(rsv, case):
    """The eight random trees of test_commit_gpu.CASES (shared groups, masks, log 0 .. 7), both sources, 1, 2 and 4 points."""
    spec, b, n, mask = CASES[case]
    ctx = rsv.Context(0)
    _check_random(ctx, spec, b, n, mask, 1300 + case)
    ctx.close()


SWITCHES = S.SWITCHES


def test_sample_tree_path_switches(rsv):
    ctx = rsv.Context(0)
    for case, (spec, b, n, mask) in enumerate(SWITCHES):
        _check_random(ctx, spec, b, n, mask, 1500 + case, ks=(1, 4) if case < 4 else (2,))
    ctx.close()


def _pass_size(spec, k, n, interpolate, budget):
    """The driver's pass size restated (sample_api.inc: sp_ws_bytes and the halving loop): per group the coefficients (from
    evaluations only), one weight table per distinct log (all groups share the points), the chunk sums; every part on a
    256-byte boundary."""
    def ws(m):
        off, seen = 0, set()
        for log, nc in spec:
            parts = [(m * nc) << log] if interpolate else []
            if log not in seen:
                parts.append(m * k * (256 + (1 << max(log - 8, 0))) * 4)
                seen.add(log)
            parts.append(m * nc * k * (1 << max(log - 13, 0)) * 4)
            for words in parts:
                off = ((off + 255) & ~255) + 4 * words
        return off
    m = n
    while ws(m) > budget and m > 1:
        m = (m + 1) // 2
    return m, ws(n)


def test_sample_under_a_small_workspace_budget(rsv):
    """41 proofs, 4 points, a log-9 group of 6 columns and a log-8 group of 11 columns that every proof shares
    (proof_stride 0), three proofs masked.  Under a 1 MB budget both sources are cut: from coefficients the workspace of the
    whole batch is 1 396 416 bytes (two weight tables of 41 x 4 x 258 and 41 x 4 x 257 entries of 16 bytes, chunk sums of
    41 x 6 x 4 and 41 x 11 x 4 entries, each part on a 256-byte boundary), so the driver halves to 21 proofs a pass (21 +
    20: the caller's buffers are read at p0 = 21, the mask at p0 + p, the shared group at stride 0); from evaluations the
    coefficients add 965 632 bytes and the passes are 11 + 11 + 11 + 8.  _pass_size restates the driver's
    arithmetic and the test asserts both figures, so it cannot go vacuous if the layout changes.  Every element of both cut
    runs equals the uncut run, and the uncut run the restatement."""
    rng = np.random.default_rng(77)
    n, k = 41, 4
    spec = [(9, 6), (8, 11)]
    budget = 1 << 20
    assert _pass_size(spec, k, n, False, budget) == (21, 1396416)
    assert _pass_size(spec, k, n, True, budget) == (11, 1396416 + 965632)
    assert _pass_size(spec, k, n, True, 8192 << 20)[0] == n and _pass_size(spec, k, n, False, 8192 << 20)[0] == n
    groups = [(9, rng.integers(0, P, (n, 6, 1 << 9))), (8, rng.integers(0, P, (1, 11, 1 << 8)))]
    mask = [0 if p in (1, 20, 40) else 1 for p in range(n)]
    pts = _points(rng, n, k)
    ctx = rsv.Context(0)
    gs = _groups_dev(groups, shared={1})
    # coefficients: the per-proof group's from a commitment, the shared group's one set (numpy) at proof_stride 0
    gc = [_coeffs_dev(ctx, gs[:1], n, 2, None)[0], _groups_dev([(8, C.interpolate(groups[1][1], 8))], shared={0})[0]]
    whole = [_sample_dev(ctx, gs, n, pts, mask, 0), _sample_dev(ctx, gc, n, pts, mask, 1)]
    ctx.set_option("ws_budget_mb", 1)
    cut = [_sample_dev(ctx, gs, n, pts, mask, 0), _sample_dev(ctx, gc, n, pts, mask, 1)]
    ctx.close()
    assert np.array_equal(whole[0], whole[1])
    assert np.array_equal(cut[0], whole[0]) and np.array_equal(cut[1], whole[0])
    for p in range(n):
        if not mask[p]:
            assert not whole[0][p].any(), p
            continue
        want = S.sample_tree([(9, groups[0][1][p]), (8, groups[1][1][0])], [_pt(pts[p, j]) for j in range(k)])
        assert np.array_equal(whole[0][p], want), p


@pytest.mark.parametrize("log", [12, 16])
def test_worst_case_ranges(rsv, log):
    """Coefficients all P - 1 (source COEFFS), the largest canonical word, at points with all words P - 1 and at random
    ones.  The weight words are products of the point's coordinates and not under the test's control, so this checks the
    values with the largest coefficients; it does not reach the edge of the u64 range, which the bound next to sp_fold
    covers for any canonical weights."""
    rng = np.random.default_rng(log)
    co = np.full((1, 2, 1 << log), P - 1, np.int64)
    pts = _points(rng, 1, 4)
    pts[0, 0] = P - 1
    ctx = rsv.Context(0)
    got = _sample_dev(ctx, _groups_dev([(log, co)]), 1, pts, None, 1)
    ctx.close()
    want = S.sample_coeffs([(log, co[0])], [_pt(pts[0, j]) for j in range(4)])
    assert np.array_equal(got[0], want)


def test_sample_at_a_domain_point_is_the_lde(rsv):
    """At a point of the LDE domain embedded in QM31 the sample of every column is (d_lde[position], 0, 0, 0) of a
    commit_tree on the same groups."""
    import torch
    dev = torch.device(DEV)
    rng = np.random.default_rng(5)
    b, n = 2, 2
    spec = [(6, 3), (9, 2), (13, 1)]
    groups = [(log, rng.integers(0, P, (n, nc, 1 << log))) for log, nc in spec]
    ctx = rsv.Context(0)
    gs = _groups_dev(groups)
    with_lde = [dict(g, d_lde=full((n, g["n_cols"], 1 << (g["log_size"] + b)))) for g in gs]
    ctx.commit_tree(with_lde, n, b, torch.zeros((n, 8), dtype=torch.int32, device=dev))
    ctx.synchronize()
    for g in with_lde:
        N = g["log_size"] + b
        pos = rng.integers(0, 1 << N, (n, 3)).astype(np.uint32)
        xy = np.stack([rsv.domain_points(N, pos[p]) for p in range(n)]).reshape(n, 3, 2)
        pts = np.zeros((n, 3, 8), np.uint32)
        pts[:, :, 0], pts[:, :, 4] = xy[:, :, 0], xy[:, :, 1]
        got = _sample_dev(ctx, [{k: v for k, v in g.items() if k != "d_lde"}], n, pts, None, 0)
        lde = u32(g["d_lde"])
        for p in range(n):
            for j in range(3):
                assert np.array_equal(got[p, j, :, 0], lde[p, :, pos[p, j]]) and not got[p, j, :, 1:].any(), (N, p, j)
    ctx.close()


def test_point_words_are_taken_mod_p(rsv):
    """Every u32 is a point word: residue + P on every word of a proof's points, residue + 2 P where that still is a u32
    (residues 0 and 1: 0xfffffffe and 0xffffffff), and P itself give what the residues give."""
    rng = np.random.default_rng(8)
    cols = rng.integers(0, P, (2, 3, 1 << 9))
    pts = _points(rng, 2, 2)
    pts[1, 0, :4] = (0, 1, 1, 0)
    pts[1, 1, 3] = 0
    big = pts.astype(np.uint64)
    big[0] += P
    big[1, 0, :4] += 2 * P
    big[1, 0, 4:] += P
    big[1, 1, 3] = P
    assert int(big.max()) == 0xFFFFFFFF and np.array_equal(big % P, pts)
    ctx = rsv.Context(0)
    gs = _groups_dev([(9, cols)])
    assert np.array_equal(_sample_dev(ctx, gs, 2, big.astype(np.uint32), None, 0), _sample_dev(ctx, gs, 2, pts, None, 0))
    ctx.close()


def test_device_refusals(rsv):
    """NULL pointers, n_points 0 and 5, an unknown source, misalignment, group sizes: the codes of the neighbouring entry
    points, nothing written."""
    import torch
    dev = torch.device(DEV)
    ctx = rsv.Context(0)
    cols = torch.zeros((1, 2, 16), dtype=torch.int32, device=dev)
    raw = torch.zeros(4096, dtype=torch.uint8, device=dev)
    g = {"log_size": 4, "d_cols": cols, "n_cols": 2}
    out = torch.full((1, 1, 2, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    pts = torch.zeros((1, 1, 8), dtype=torch.int32, device=dev)

    def refused(code, groups=(g,), d_points=pts, k=1, d_samples=out, source=0):
        with pytest.raises(rsv.RsvError) as e:
            ctx.sample_tree(list(groups), 1, d_points, k, d_samples, source=source)
        assert e.value.code == code, (code, e.value.code)

    refused(-1, d_points=None)
    refused(-1, d_samples=None)
    refused(-1, groups=[dict(g, d_cols=None)])
    refused(-2, k=0)
    refused(-2, k=5)
    refused(-2, source=2)
    refused(-2, groups=[g] * 9)
    refused(-2, groups=[dict(g, n_cols=0)])
    refused(-2, groups=[dict(g, log_size=30)])
    refused(-2, groups=[dict(g, d_cols=raw[1:])])
    refused(-2, d_points=raw[1:33])
    refused(-2, d_samples=raw[2:34])
    ctx.synchronize()
    assert bool((out == 0x5A5A5A5A).all())
    ctx.sample_tree([g], 1, pts, 1, out)
    ctx.synchronize()
    assert not bool(out.any())  # zero columns: zero samples, every word written
    ctx.close()
