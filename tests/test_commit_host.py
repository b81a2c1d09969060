"""Commitment of trees 0, 1 and 2 of the next proof (no device).  The numpy restatement in tests/commit_ref.py (circle
interpolation and LDE, the mixed-size Merkle tree hashed by the oracle, the transcript prefix) is pinned to the reference
on the cheapest fixture pair, recursive_proof_16_15 x5 -> level1-5 (LDE sizes 2^20 / 2^19), with the columns of the
oracle's circuit: its three roots are level1-5's commitments[0..2], its LDE at the query positions is what level1-5
decommits, and its transcript draws are level1-5's.  tests/test_commit_gpu.py compares the device against this helper.
Also: the argument refusals of the new entry points that need no device."""
import ctypes

import numpy as np

from tests import commit_ref as C
from tests import interaction_ref as R
from tests import oracle_binding as ob
from tests.conftest import fixture_cfg, read_proof
from tests.chain_harness import inputs_of, oracle_columns

P = C.P


def test_restatement_reproduces_the_next_fixture():
    from oracle import recursion_circuit as rc
    ppre, ptr, qpre, qtr, lp, lq, dst = oracle_columns("recursive_proof_16_15.bin")
    nxt = read_proof(dst)
    b = fixture_cfg(dst).log_blowup_factor
    d = rc.parse_proof(nxt)
    tr = ob.transcript_raw(nxt)
    z, alpha = tuple(int(x) for x in tr[4:8]), tuple(int(x) for x in tr[8:12])
    # the draws come from the restated roots: tree 2 needs (z, alpha) only through them
    roots = []
    cols = ob.trace_cols(nxt, inputs_of(dst))
    qM, M = C.query_positions(nxt, ob)
    trees = [[(lp, ppre), (lq, qpre)], [(lp, ptr), (lq, qtr)], None]
    for t in range(3):
        if t == 2:
            zz, aa, _, _ = C.transcript_prefix(roots + [np.zeros(8, np.uint32)], lp, lq, ((0,) * 4, (0,) * 4), ob)
            assert (zz, aa) == (z, alpha)
            cp, cq, sums, ok = R.interaction(ppre, ptr, qpre, qtr, zz, aa, lp, lq)
            assert ok
            trees[2] = [(lp, cp), (lq, cq)]
        layers = C.tree_layers(trees[t], b)
        roots.append(C.merkle_root(layers, ob))
        assert roots[t].tolist() == [int(x) for x in d.commitments[t]], t
        top = max(layers)
        for j in (0, 1, len(qM) - 1):
            got = C.decommitted(layers, int(qM[j]) >> (M - top))
            assert got == cols[t, j, :len(got)].tolist(), (t, j)
        del layers
    z2, a2, rcoeff, ch = C.transcript_prefix(roots, lp, lq, sums, ob)
    assert (z2, a2) == (z, alpha) and rcoeff == tuple(int(x) for x in tr[12:16])
    ch.mix([int(x) for x in d.commitments[3]])
    assert ch.draw()[0] == tuple(int(x) for x in tr[16:20])


def test_interpolate_evaluate_round_trip():
    """LDE then interpolation on the larger domain: the coefficients, zero-padded; eval_at_point of the coefficients at a
    domain point is the stored value."""
    rng = np.random.default_rng(3)
    for log in (0, 1, 2, 5):
        col = rng.integers(0, P, 1 << log)
        co = C.interpolate(col, log)
        assert np.array_equal(C.evaluate(co, log, log), col % P)
        big = C.lde(col, log, 3)
        co2 = C.interpolate(big, log + 3)
        assert np.array_equal(co2[:1 << log], co) and not co2[1 << log:].any()
    col = rng.integers(0, P, 32)
    co = C.interpolate(col, 5)
    from oracle.recursion_circuit import gadgets as G
    half = G.canonic_half_coset(5)
    pt = G.point_of_index(half.initial_index + int(C.bit_reverse(3, 4)) * half.step_size)  # position 6 = 2 * 3: domain index bitrev(3)
    assert C.eval_at_point(co, 5, ((pt[0], 0, 0, 0), (pt[1], 0, 0, 0))) == (int(col[6]), 0, 0, 0)


def test_argument_validation_needs_no_device(rsv):
    """Refusals that return before any device work: NULL context / groups / columns, log_blowup 0 or above the limit,
    log + b above RSV_MAX_LOG_SIZE, too many groups, an unbuilt program for the host chain."""
    lib = rsv.lib
    assert all(k in rsv.EXPORTS for k in ("rsv_commit_tree_dev", "rsv_witness_commit_dev", "rsv_witness_commit"))
    fake = ctypes.create_string_buffer(64)  # never dereferenced: every refusal below comes first
    fake_p = ctypes.cast(fake, ctypes.c_void_p)
    cols = ctypes.c_void_p(4096)
    roots = ctypes.c_void_p(8192)

    def groups(*specs):
        arr = (rsv.CommitGroup * len(specs))()
        for k, (log, nc, ptr) in enumerate(specs):
            arr[k] = rsv.CommitGroup(log, nc, ptr, nc << log, None, None)
        return arr

    g = groups((4, 2, cols))
    assert lib.rsv_commit_tree_dev(None, g, 1, 1, 2, None, roots) == -1
    assert lib.rsv_commit_tree_dev(fake_p, None, 1, 1, 2, None, roots) == -1
    assert lib.rsv_commit_tree_dev(fake_p, g, 1, 1, 2, None, None) == -1
    assert lib.rsv_commit_tree_dev(fake_p, groups((4, 2, None)), 1, 1, 2, None, roots) == -1
    assert lib.rsv_commit_tree_dev(fake_p, g, 1, 1, 0, None, roots) == -2
    assert lib.rsv_commit_tree_dev(fake_p, g, 1, 1, 17, None, roots) == -2
    assert lib.rsv_commit_tree_dev(fake_p, groups((28, 2, cols)), 1, 1, 3, None, roots) == -2
    assert lib.rsv_commit_tree_dev(fake_p, groups(*[(4, 2, cols)] * 9), 9, 1, 2, None, roots) == -2
    assert lib.rsv_commit_tree_dev(fake_p, g, 0, 1, 2, None, roots) == -2
    assert lib.rsv_commit_tree_dev(fake_p, groups((4, 0, cols)), 1, 1, 2, None, roots) == -2
    assert lib.rsv_commit_tree_dev(fake_p, groups((4, 2, ctypes.c_void_p(4098))), 1, 1, 2, None, roots) == -2
    assert lib.rsv_witness_commit_dev(None, None, None, None, None, None, 0, 2, None, None, None, None, None, None, None) == -1
    assert lib.rsv_witness_commit_dev(fake_p, fake_p, cols, cols, cols, cols, 1, 0, roots, roots, roots, roots, roots, None, None) == -2
    assert lib.rsv_witness_commit(None, None, None, 0, None, None, 0, 2, None, None, None, None, None, None, 0) == -1
    assert lib.rsv_witness_commit(fake_p, None, None, 0, None, None, 0, 0, None, None, None, None, None, None, 0) == -2
    assert lib.rsv_witness_commit(fake_p, None, None, 0, None, None, 0, 17, None, None, None, None, None, None, 0) == -2
