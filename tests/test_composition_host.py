"""Tree 3 of the next proof, the composition polynomial (no device).  The conventions of tests/composition_ref.py are pinned
to the reference on the cheapest fixture pair, recursive_proof_16_15 x5 -> level1-5, with the columns of the oracle's
circuit and tests/interaction_ref.py's interaction columns, at three of level1-5's query positions: the accumulator of the
mask values at the query's domain point p equals left(p) + pi^(clb-2)(p.x) * right(p) formed from level1-5's own
queried_values[3].  That single equality checks the row definition, the previous-row offset, the accumulation order, the
claimed-sum shift and the cut against the reference without the full domain.

Where the mask values come from.  Tree 3's LDE is the proof's largest layer (L3 + b bits), so a query position is a
position of tree 3 itself, and its point p is a point of CanonicCoset(L3 + b).circle_domain().  The columns of trees 0-2
are smaller: what level1-5 decommits for them at that query (ob.trace_cols) are their values at the position shifted
down, that is at pi^k(p), not at p, and cannot serve as mask values at p.  The mask values are therefore the columns'
interpolants at p (eval_m31, pinned here to C.eval_at_point, which also gives the eight previous-row values), and
ob.trace_cols pins those same interpolants, at the shifted positions' points, to what level1-5 decommits for trees 0-2.
Also: the refusals of the new entry points that need no device."""
import ctypes

import numpy as np

from tests import commit_ref as C
from tests import composition_ref as K
from tests import interaction_ref as R
from tests import oracle_binding as ob
from tests.conftest import fixture_cfg, read_proof
from tests.chain_harness import inputs_of, oracle_columns

P = C.P


def _point(N, pos, minus_step_of=None):
    k = int(K.domain_indices(N, [pos])[0])
    if minus_step_of is not None:
        k -= 1 << (31 - minus_step_of)
    x, y = C.gen_mul([k])
    return int(x[0]), int(y[0])


def test_restatement_reproduces_the_next_fixture():
    ppre, ptr, qpre, qtr, lp, lq, dst = oracle_columns("recursive_proof_16_15.bin")
    nxt = read_proof(dst)
    b = fixture_cfg(dst).log_blowup_factor
    tr = ob.transcript_raw(nxt)
    z, alpha = tuple(int(v) for v in tr[4:8]), tuple(int(v) for v in tr[8:12])
    cp, cq, sums, ok = R.interaction(ppre, ptr, qpre, qtr, z, alpha, lp, lq)
    assert ok
    clb = K.clb_of(lp, lq)
    L3 = clb - 1
    qM, M = C.query_positions(nxt, ob)
    assert M == L3 + b  # tree 3 is the largest layer: a query position is its own
    queried = ob.trace_cols(nxt, inputs_of(dst))
    plonk = [C.interpolate(c, lp) for c in (ppre, ptr, cp)]
    poseidon = [C.interpolate(c, lq) for c in (qpre, qtr, cq)]
    for j in (0, 1, len(qM) - 1):
        q = int(qM[j])
        x, y = _point(M, q)
        vp = [K.eval_m31(c, lp, x, y) for c in plonk]
        vq = [K.eval_m31(c, lq, x, y) for c in poseidon]
        prev = []
        for log, co, v in ((lp, plonk[2], vp[2]), (lq, poseidon[2], vq[2])):
            px, py = _point(M, q, minus_step_of=log)
            prev.append([C.eval_at_point(co[k], log, ((px, 0, 0, 0), (py, 0, 0, 0))) for k in range(4, 8)])
            assert all(w[1:] == (0, 0, 0) for w in prev[-1])
            prev[-1] = np.array([[w[0]] for w in prev[-1]])
            # eval_m31 is eval_at_point
            assert C.eval_at_point(co[7], log, ((x, 0, 0, 0), (y, 0, 0, 0))) == (int(v[7]), 0, 0, 0)
        # the same interpolants at the shifted positions' points are what level1-5 decommits for trees 0, 1 and 2
        for t in range(3):
            got = []
            for log, co in sorted(((lp, plonk[t]), (lq, poseidon[t])), key=lambda e: -e[0]):
                sx, sy = _point(log + b, q >> (M - log - b))
                got.extend(int(v) for v in K.eval_m31(co, log, sx, sy))
            assert got == queried[t, j, :len(got)].tolist(), (t, j)
        samples = K.sample_vectors([v[:, None] for v in vp], [v[:, None] for v in vq], prev[0], prev[1])
        acc = K.accumulator(samples, lp, lq, sums, tr[4:16], [x])[0]
        c3 = queried[3, j, :8].astype(np.int64)
        fold = x
        for _ in range(clb - 2):
            fold = (2 * fold * fold - 1) % P
        want = (c3[:4] + c3[4:] * fold) % P
        assert acc.tolist() == want.tolist(), j


def test_previous_row_positions():
    """The previous row of a position, found through the points' indices, is a permutation that moves every point by one
    step of CanonicCoset(log) and stays inside the aligned 2^(log + 1) positions the device streams in."""
    for N, log in ((6, 4), (8, 3), (8, 5), (7, 5)):
        prev = K.prev_positions(N, log)
        assert sorted(prev.tolist()) == list(range(1 << N))
        assert np.array_equal(prev >> (log + 1), np.arange(1 << N) >> (log + 1))
        k = K.domain_indices(N)
        assert np.array_equal((k - k[prev]) & ((1 << 31) - 1), np.full(1 << N, 1 << (31 - log)))


def test_argument_validation_needs_no_device(rsv):
    """Refusals that return before any device work: NULL pointers, lp or lq below 2, clb above RSV_MAX_LOG_SIZE, n above
    2^20, misalignment; rsv_composition_log_size is host arithmetic."""
    lib = rsv.lib
    assert all(k in rsv.EXPORTS for k in ("rsv_composition_log_size", "rsv_composition_dev", "rsv_witness_tree3_dev"))
    assert rsv.composition_log_size(4, 3) == 5 and rsv.composition_log_size(3, 5) == 7 and rsv.composition_log_size(11, 10) == 12
    assert rsv.composition_log_size(28, 27) == 29
    out = ctypes.c_uint32(77)
    assert lib.rsv_composition_log_size(4, 3, None) == -1
    assert lib.rsv_composition_log_size(1, 3, ctypes.byref(out)) == -2 and lib.rsv_composition_log_size(3, 1, ctypes.byref(out)) == -2
    assert lib.rsv_composition_log_size(29, 3, ctypes.byref(out)) == -2 and lib.rsv_composition_log_size(3, 28, ctypes.byref(out)) == -2
    assert out.value == 77
    fake = ctypes.create_string_buffer(64)  # never dereferenced: every refusal below comes first
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    a = ctypes.c_void_p(4096)

    def comp(ctx=ctx, lp=4, lq=3, ptrs=(a,) * 6, sums=a, draws=a, n=1, d_comp=a, d_coeffs=None):
        cols = []
        for ptr in ptrs:
            cols += [ptr, 0]
        return lib.rsv_composition_dev(ctx, lp, lq, *cols, sums, draws, None, n, d_comp, d_coeffs)

    assert comp(ctx=None) == -1
    for k in range(6):
        assert comp(ptrs=(a,) * k + (None,) + (a,) * (5 - k)) == -1
    assert comp(sums=None) == -1 and comp(draws=None) == -1 and comp(d_comp=None) == -1
    assert comp(lp=1) == -2 and comp(lq=1) == -2 and comp(lp=29) == -2 and comp(lq=28) == -2
    assert comp(n=(1 << 20) + 1) == -2
    odd = ctypes.c_void_p(4098)
    for k in range(6):
        assert comp(ptrs=(a,) * k + (odd,) + (a,) * (5 - k)) == -2
    assert comp(sums=odd) == -2 and comp(draws=odd) == -2 and comp(d_comp=odd) == -2 and comp(d_coeffs=odd) == -2
    assert comp(n=0) == 0

    def tree3(ctx=ctx, prog=ctx, b=2, ptrs=(a,) * 13, cap=None):
        plonk, pos, ops, ip, iq, acc, sums, draws, chan, d_comp, root, oods, smp = ptrs
        return lib.rsv_witness_tree3_dev(ctx, prog, plonk, pos, ops, ip, iq, acc, None, 1, b, sums, draws, chan, d_comp, root, cap, oods, smp)

    assert tree3(ctx=None) == -1 and tree3(prog=None) == -1
    for k in range(13):
        if k != 2:  # d_ops may be NULL for a program without witness ops
            assert tree3(ptrs=(a,) * k + (None,) + (a,) * (12 - k)) == -1, k
    assert tree3(b=0) == -2 and tree3(b=17) == -2
    for k in range(13):
        assert tree3(ptrs=(a,) * k + (odd,) + (a,) * (12 - k)) == -2, k
    assert tree3(cap=odd) == -2
