"""The interaction (logup) columns, tree 2 of the next proof (no device).  The numpy restatement in tests/interaction_ref.py,
built from the oracle's own columns (oracle/recursion_circuit/trace.py), is pinned to the reference: fixture K+1's two
claimed sums and its 24 tree-2 sampled values (16 at the OODS point, 8 at the previous-row point) with K+1's own (z,
alpha).  tests/test_interaction_gpu.py compares the device against this helper.  Also: the balance identity for random
lookup elements, and the argument checks of rsv_witness_interaction(_dev) that need no device."""
import ctypes

import numpy as np
import pytest

from tests import interaction_ref as R
from tests.conftest import load_manifest, read_proof
from tests.chain_harness import lookup_of, oods_of, oracle_columns

P = R.P
MAN = {e["file"]: e for e in load_manifest()}


def tree2_samples(cp, cq, lp, lq, oods):
    """The 24 sampled values of tree 2 in the proof's order: per column [oods] (columns 0..3) or [prev row, oods]."""
    from oracle.recursion_circuit import trace as T
    out = []
    for log, cols in ((lp, cp), (lq, cq)):
        ev = T.PointEvaluator(log, oods)
        evp = T.PointEvaluator(log, R.prev_row_point(oods, log))
        for k in range(8):
            out.append([ev.eval(cols[k])] if k < 4 else [evp.eval(cols[k]), ev.eval(cols[k])])
    return out


@pytest.mark.parametrize("src", ["small_proof.bin", "level10-1.bin"])
def test_restatement_reproduces_the_next_fixture(src):
    """Claimed sums (stmt1) and all 24 tree-2 sampled values of fixture K+1, bit for bit, with K+1's (z, alpha)."""
    from oracle import recursion_circuit as rc
    ppre, ptr, qpre, qtr, lp, lq, dst = oracle_columns(src)
    z, alpha = lookup_of(dst)
    cp, cq, sums, ok = R.interaction(ppre, ptr, qpre, qtr, z, alpha, lp, lq)
    assert ok
    d = rc.parse_proof(read_proof(dst))
    assert sums == (tuple(d.plonk_total_sum), tuple(d.poseidon_total_sum))
    want = [[tuple(v) for v in col] for col in d.sampled_values[2]]
    assert len(want) == 16 and sum(len(c) for c in want) == 24
    assert tree2_samples(cp, cq, lp, lq, oods_of(dst)) == want
    # the cumulative column ends at zero in coset order
    for cols, log in ((cp, lp), (cq, lq)):
        last = R.coset_positions(log)[-1]
        assert not cols[4:, last].any()


def test_balance_identity_for_random_lookup_elements():
    """plonk + poseidon + sum over the public inputs of 1 / (v + idx alpha - z) = 0 for any (z, alpha)."""
    ppre, ptr, qpre, qtr, lp, lq, dst = oracle_columns("small_proof.bin")
    inputs = [(i, tuple(v)) for i, v in MAN[dst]["inputs"]]  # the circuit's: variables 1, 2, 3 = 1, i, j
    rng = np.random.default_rng(7)
    for _ in range(3):
        z, alpha = (tuple(int(x) for x in rng.integers(0, P, 4)) for _ in range(2))
        _, _, (sp, sq), ok = R.interaction(ppre, ptr, qpre, qtr, z, alpha, lp, lq)
        assert ok
        total = R.q_add(R.q_add(R.q(sp), R.q(sq)), R.q(R.input_sum(inputs, z, alpha)))
        assert not total.any()


def test_coset_positions_are_a_permutation():
    for log in (1, 2, 5, 10):
        pos = R.coset_positions(log)
        assert sorted(pos.tolist()) == list(range(1 << log))
    # n = 2: coset indices 0, 1, 2, 3 sit at circle-domain indices 0, 3, 1, 2, stored bit-reversed at 0, 3, 2, 1
    assert R.coset_positions(2).tolist() == [0, 3, 2, 1]


def test_argument_validation_needs_no_device(rsv):
    """NULL and unbuilt programs are refused before any device work."""
    lib = rsv.lib
    assert lib.rsv_witness_interaction_dev(None, None, None, None, None, None, 0, None, None, None, None) == -1
    assert lib.rsv_witness_interaction(None, None, None, 0, None, None, 0, None, None, None, None, None, None, None, 0) == -1
    # a batch with outputs missing: NULL before anything else
    blob = np.zeros(16, np.uint8)
    offs = np.array([0, 16], np.uint64)
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    assert lib.rsv_witness_interaction(None, blob.ctypes.data_as(u8p), offs.ctypes.data_as(u64p), 1, None, None, 0, None, None, None, None,
                                       None, None, None, 0) == -1
    assert "rsv_witness_interaction_dev" in rsv.EXPORTS and "rsv_witness_interaction" in rsv.EXPORTS


def test_lookup_argument_shapes(rsv):
    """One (z, alpha) for the whole batch or one per proof; anything else is refused."""
    one = ((1, 2, 3, 4), (5, 6, 7, P + 8))
    arr = rsv._lookup_array(one, 3)
    assert arr.shape == (3, 8) and arr[2].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    per = np.arange(16).reshape(2, 2, 4)
    assert rsv._lookup_array(per, 2).tolist() == [list(range(8)), list(range(8, 16))]
    with pytest.raises(rsv.RsvError) as e:
        rsv._lookup_array(per, 3)
    assert e.value.code == -2
