"""Sampled values of trees 0, 1 and 2 of the next proof (no device).  The numpy restatement in tests/sample_ref.py is pinned
(a) to the reference: with the columns of the oracle's circuit and K+1's OODS point its `witness_samples` is K+1's
sampled_values[0..2], all 134 values in the proof's order, for the pairs the commitment's and the interaction's host tests
already build (small_proof, recursive_proof_16_15 x5, level10-1); (b) to the definition: its dot-product form equals
commit_ref.eval_at_point and the oracle's PointEvaluator on random columns at random points off the circle.
tests/test_sample_gpu.py compares the device against this helper.  Also: the argument refusals of rsv_sample_tree_dev and
rsv_witness_sample_dev, which need no device."""
import ctypes

import numpy as np
import pytest

from tests import commit_ref as C
from tests import interaction_ref as R
from tests import sample_ref as S
from tests.conftest import read_proof
from tests.chain_harness import lookup_of, oods_of, oracle_columns

P = C.P


@pytest.mark.parametrize("src", ["small_proof.bin", "recursive_proof_16_15.bin", "level10-1.bin"])
def test_restatement_reproduces_the_next_fixture_samples(src):
    from oracle import recursion_circuit as rc
    ppre, ptr, qpre, qtr, lp, lq, dst = oracle_columns(src)
    z, alpha = lookup_of(dst)
    cp, cq, _, ok = R.interaction(ppre, ptr, qpre, qtr, z, alpha, lp, lq)
    assert ok
    trees = [[(lp, ppre), (lq, qpre)], [(lp, ptr), (lq, qtr)], [(lp, cp), (lq, cq)]]
    got = S.witness_samples(trees, oods_of(dst))
    d = rc.parse_proof(read_proof(dst))
    want = S.flatten_samples(d.sampled_values)
    assert [len(d.sampled_values[t]) for t in range(3)] == [50, 60, 16] and want.shape == (134, 4)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0].tolist()


def _point(rng):
    return tuple(int(v) for v in rng.integers(0, P, 4)), tuple(int(v) for v in rng.integers(0, P, 4))


@pytest.mark.parametrize("log", range(11))
def test_dot_product_form_is_eval_at_point(log):
    """Random coefficients, random points (not on the circle): weights . coefficients = CirclePoly::eval_at_point; with
    evaluations in, = the oracle's PointEvaluator (defined from log 1 on: it folds the evaluations, no interpolation)."""
    from oracle.recursion_circuit import trace as T
    rng = np.random.default_rng(40 + log)
    cols = rng.integers(0, P, (3, 1 << log))
    pts = [_point(rng), _point(rng)]
    co = C.interpolate(cols, log)
    got = S.sample_tree([(log, cols)], pts)
    assert got.shape == (2, 3, 4)
    assert np.array_equal(got, S.sample_coeffs([(log, co)], pts))
    for k, pt in enumerate(pts):
        ev = T.PointEvaluator(log, pt) if log >= 1 else None
        for c in range(3):
            want = C.eval_at_point(co[c], log, pt)
            assert tuple(got[k, c].tolist()) == want, (k, c)
            if ev is not None:
                assert tuple(int(v) for v in ev.eval(cols[c])) == want, (k, c)
    # point words are taken mod P
    big = (tuple(v + P for v in pts[0][0]), tuple(v + (P if i & 1 else 0) for i, v in enumerate(pts[0][1])))
    assert np.array_equal(S.sample_tree([(log, cols)], [big])[0], got[0])


def test_worst_case_words():
    """Coefficients and point words all P - 1: the restatement's sums stay exact (products are reduced before they are added)."""
    top = ((P - 1,) * 4, (P - 1,) * 4)
    for log in (4, 12):
        co = np.full((1, 1 << log), P - 1, np.int64)
        assert tuple(S.sample_coeffs([(log, co)], [top])[0, 0].tolist()) == C.eval_at_point(co[0], log, top)


def test_argument_validation_needs_no_device(rsv):
    """Every refusal of rsv_sample_tree_dev and rsv_witness_sample_dev returns before any device work; with valid arguments
    and no device the answer is RSV_E_DEVICE."""
    lib = rsv.lib
    assert "rsv_sample_tree_dev" in rsv.EXPORTS and "rsv_witness_sample_dev" in rsv.EXPORTS
    assert (rsv.SAMPLE_COLUMNS, rsv.SAMPLE_COEFFS, rsv.MAX_SAMPLE_POINTS) == (0, 1, 4)
    fake = ctypes.create_string_buffer(8192)  # zeros: device 0; the refusals below come before anything else is read
    fake_p = ctypes.cast(fake, ctypes.c_void_p)
    fake_prog = ctypes.create_string_buffer(8192)
    prog_p = ctypes.cast(fake_prog, ctypes.c_void_p)
    buf, odd = ctypes.c_void_p(8192), ctypes.c_void_p(8194)

    def groups(*specs):
        arr = (rsv.CommitGroup * len(specs))()
        for k, (log, nc, ptr) in enumerate(specs):
            arr[k] = rsv.CommitGroup(log, nc, ptr, nc << log, None, None)
        return arr

    g = groups((4, 2, ctypes.c_void_p(4096)))

    def call(ctx=fake_p, gr=g, ng=1, n=1, source=0, pts=buf, npts=1, out=buf):
        return lib.rsv_sample_tree_dev(ctx, gr, ng, n, None, source, pts, npts, out)

    assert call(ctx=None) == -1 and call(gr=None) == -1 and call(pts=None) == -1 and call(out=None) == -1
    assert call(gr=groups((4, 2, None))) == -1
    assert call(npts=0) == -2 and call(npts=5) == -2
    assert call(source=2) == -2 and call(source=-1) == -2
    assert call(ng=0) == -2 and call(gr=groups(*[(4, 2, ctypes.c_void_p(4096))] * 9), ng=9) == -2
    assert call(gr=groups((4, 0, ctypes.c_void_p(4096)))) == -2 and call(gr=groups((30, 1, ctypes.c_void_p(4096)))) == -2
    assert call(n=(1 << 20) + 1) == -2
    assert call(pts=odd) == -2 and call(out=odd) == -2 and call(gr=groups((4, 2, ctypes.c_void_p(4098)))) == -2
    assert call(n=0) == 0  # an empty batch is no work

    def chain(ctx=fake_p, prog=prog_p, plonk=buf, pos=buf, ops=buf, ip=buf, iq=buf, acc=buf, ok=None, n=1, oods=buf, out=buf):
        return lib.rsv_witness_sample_dev(ctx, prog, plonk, pos, ops, ip, iq, acc, ok, n, oods, out)

    for name in ("ctx", "prog", "plonk", "pos", "ip", "iq", "acc", "oods", "out"):
        assert chain(**{name: None}) == -1, name
    for name in ("plonk", "pos", "ops", "ip", "iq", "oods", "out"):
        assert chain(**{name: odd}) == -2, name
    assert chain(n=(1 << 20) + 1) == -2
    if rsv.device_count() == 0:
        assert call() == -3 and call(source=1, npts=4) == -3
        assert chain() == -3
