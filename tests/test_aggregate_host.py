"""tests/aggregate_ref.py pinned on the CPU: the oracle's circuit of a group of DIFFERENT proofs, which the GPU tests of the
aggregation (tests/test_aggregate_gpu.py) compare against.  Without this they could silently compare against a same-proof
circuit."""
import numpy as np

from tests import aggregate_ref as R
from tests.aggregate_ref import A, B


def test_mixed_circuit_is_a_circuit_and_its_blocks_are_the_members():
    """[A, B] (level10-1.bin, level11-1.bin: one shape, one configuration) in one constraint system: every gate holds; copy 0
    is variables [0, 47 788) and equals that block of [A, A], copy 1 is [47 788, 95 537) and equals that block of [B, B]; the
    two proofs differ in 44 578 variables of the first block; 7 564 invocations (3 782 per copy); 2^17 Plonk rows after pad().
    Only the op column (the witness-dependent gate constants) differs between the mixed circuit and [A, A]: no wire does."""
    import copy

    from oracle.recursion_circuit import trace as T
    mixed, marks = R.circuit((A, B))
    mixed.check_arithmetics()
    aa, marks_aa = R.circuit((A, A))
    bb, marks_bb = R.circuit((B, B))
    assert marks == marks_aa == marks_bb == [4, 47788, 95537]  # (the four fixed constants precede copy 0)
    v, va, vb = (np.array(c.variables, dtype=np.uint32) for c in (mixed, aa, bb))
    m = marks[1]
    assert np.array_equal(v[:m], va[:m]) and np.array_equal(v[m:], vb[m:])
    assert int((va[:m] != vb[:m]).any(axis=1).sum()) == 44578
    assert not np.array_equal(v[m:], va[m:])  # the second copy is B's, not A's again
    assert len(mixed.flow) == 7564 == 2 * 3782
    for name in ("a_wire", "b_wire", "c_wire", "poseidon_wire", "enforce_c_m31"):
        assert getattr(mixed, name) == getattr(aa, name), name
    assert mixed.op != aa.op
    assert [tuple(x[0] for x in e[:4]) + (e[4],) for e in mixed.flow] == [tuple(x[0] for x in e[:4]) + (e[4],) for e in aa.flow]
    assert T.pad(copy.deepcopy(mixed)) == 1 << 17


def test_the_order_of_the_members_is_the_order_of_the_blocks():
    """[B, A] is [A, B] with the members' blocks exchanged where they are hints: its first block is [B, B]'s, its second
    [A, A]'s."""
    ba, marks = R.circuit((B, A))
    ba.check_arithmetics()
    m = marks[1]
    v = np.array(ba.variables, dtype=np.uint32)
    assert np.array_equal(v[:m], R.variables((B, B))[:m]) and np.array_equal(v[m:], R.variables((A, A))[m:])
    assert not np.array_equal(v, R.variables((A, B)))
