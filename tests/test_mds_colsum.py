"""The external linear layer with the column sums formed first (PermT::colsums_2x, mds4, mds_group_2x and the half-output
tail of poseidon2_inline_half, recursive-stwo_amd/csrc/poseidon2.hpp) on machine words.

circ(2M4, M4, M4, M4) s has group g equal to M4 s_g + M4 X with X_j = s_j + s_{4+j} + s_{8+j} + s_{12+j}, and M4 is linear, so
the header forms z_g = s_g + X first and applies one M4 per group to 64-bit inputs.  ColSum restates that statement by
statement on the accumulator instructions of tests/perm_model.py (every v_mad_u64_u32 and v_lshl_add_u64 result asserted
below 2^64) and is compared with perm_model's layer, which applies M4 to each group first and adds the sums of its outputs
afterwards: the 16 doubled accumulators V[i] must be the same integers, so nothing downstream of the layer moves."""
import re

import numpy as np

from tests import oracle_binding as ob
from tests import perm_model as pm
from tests.perm_model import M32, P

W = 1 << 32
# the reference's known answer for the state 0..15
KAT_OUT = [260776483, 1182896747, 1656699352, 746018898, 102875940, 1812541025, 515874083, 755063943, 1682438524, 1265420601,
           238640995, 200799880, 1659717477, 2080202267, 1269806256, 1287849264]


class ColSum(pm.Model):
    """perm_model.Model with the header's layer; `seen` keeps the largest value of every named intermediate, `ops` counts
    the instructions by kind."""

    def __init__(self, *a):
        super().__init__(*a)
        self.seen, self.ops = {}, {"mul": 0, "mad": 0, "lshl_add": 0}

    def _see(self, name, v):
        self.seen[name] = max(self.seen.get(name, 0), v)
        return v

    def mad(self, a, b, c=None):
        self.ops["mul" if c is None else "mad"] += 1
        return super().mad(a, b, 0 if c is None else c)

    def add64(self, a, b, sh=0):
        self.ops["lshl_add"] += 1
        return super().add64(a, b, sh)

    def colsums_2x(self, s):
        X2 = [self.mad(s[j], 2) for j in range(4)]
        for g in range(1, 4):
            X2 = [self.mad(s[4 * g + j], 2, X2[j]) for j in range(4)]
        return [self._see("X2", x) for x in X2]

    def mds4(self, z0, z1, z2, z3):
        t0, t1 = self._see("t0", self.add64(z0, z1)), self._see("t1", self.add64(z2, z3))
        t2, t3 = self._see("t2", self.add64(z1, t1, 1)), self._see("t3", self.add64(z3, t0, 1))
        t4, t5 = self._see("t4", self.add64(t1, t3, 2)), self._see("t5", self.add64(t0, t2, 2))
        return [self._see("V", v) for v in (self.add64(t3, t5), t5, self.add64(t2, t4), t4)]

    def mds_group_2x(self, X2, x):
        return self.mds4(*[self._see("z", self.mad(x[j], 2, X2[j])) for j in range(4)])

    def mds16_2x(self, s):
        X2 = self.colsums_2x(s)
        return [v for g in range(4) for v in self.mds_group_2x(X2, s[4 * g:4 * g + 4])]

    def half_tail(self, s, hi):
        """poseidon2_inline_half<HI> after poseidon2_rounds: the eight canonical words of one half"""
        X2 = self.colsums_2x(s)
        out = []
        for g in range(2):
            for v in self.mds_group_2x(X2, s[(8 if hi else 0) + 4 * g:][:4]):
                t = self.fold2(v)
                assert t <= P + self.hi_full
                out.append(self.ar.canon(t))
        return out


def _models():
    args = (pm.Exact, pm.constants(), *pm.header())
    return ColSum(*args), pm.Model(*args)


def _one_hot(i, v):
    return [v if k == i else 0 for k in range(16)]


def test_accumulators_equal_the_sum_after_m4_form():
    new, old = _models()
    rng = np.random.default_rng(181)
    states = [[0] * 16, [M32] * 16, [2 * P - 1] * 16] + [_one_hot(i, M32) for i in range(16)]
    states += rng.integers(0, W, (10_000, 16), dtype=np.uint64).tolist()
    for st in states:
        assert new.mds16_2x(st) == old.mds16_2x(st), st


def test_instruction_counts_of_the_layer_and_the_tail():
    """The restatement above costs what the change was priced at: 64 instructions a layer, 40 the tail.  These are the
    model's counts; the header's own are read off the compiler's listing by tools/perm_ceiling.py."""
    new, _ = _models()
    new.mds16_2x([1] * 16)
    assert new.ops == {"mul": 4, "mad": 28, "lshl_add": 32}
    new.ops = dict.fromkeys(new.ops, 0)
    new.half_tail([1] * 16, True)
    assert new.ops == {"mul": 4, "mad": 20, "lshl_add": 16}


def test_interval_bounds_with_every_input_at_the_largest_word():
    """Every operation is monotone in its inputs, so the values at all-0xFFFFFFFF bound every state of u32 words."""
    new, _ = _models()
    V = new.mds16_2x([M32] * 16)
    limit = {"X2": 1 << 35, "z": 1 << 36, "t0": 1 << 37, "t1": 1 << 37, "t2": 40 * W, "t3": 40 * W, "t4": 120 * W, "t5": 120 * W,
             "V": 160 * W}
    assert set(new.seen) == set(limit)
    for name, top in limit.items():
        assert new.seen[name] < top <= 1 << 40, name
    assert max(V) < 160 * W and max(V) >> 32 < new.hi_full
    assert max(new.fold2(v) for v in V) <= P + new.hi_full
    # the figures above are the ones the header states
    src = open(pm.HDR).read()
    for line in (r"X2_j = 2 X_j\s+< 4 \* 2\^33 = 2\^35", r"z_j  = 2 s_\{4g\+j\} \+ X2_j\s+< 10 \* 2\^32 < 2\^36",
                 r"t0, t1 < 2\^37;  t2, t3 < 40 \* 2\^32;  t4, t5 < 120 \* 2\^32;  y_j < 160 \* 2\^32 < 2\^40"):
        assert re.search(line, src), line
    assert "mds4_2x" not in src


def test_half_tail_equals_the_full_layer():
    """Both halves against the full layer's words after fold and canonicalisation, on L2-range states and on states whose
    accumulators are non-zero multiples of 2P: those fold to P itself, which canonicalises to 0."""
    new, old = _models()
    rng = np.random.default_rng(182)
    multiples = [[P] * 16, [P if i % 2 else 0 for i in range(16)], [2 * P if i < 4 else 0 for i in range(16)], _one_hot(9, P)]
    for st in multiples:
        folds = [old.fold2(v) for v in old.mds16_2x(st)]
        assert folds == [P] * 16, st
    states = multiples + [[0] * 16, [2 * P - 1] * 16] + rng.integers(0, 2 * P, (2_000, 16), dtype=np.uint64).tolist()
    for st in states:
        want = [pm.Exact.canon(old.fold2(v)) for v in old.mds16_2x(st)]
        assert max(want) < P
        assert new.half_tail(st, False) == want[:8] and new.half_tail(st, True) == want[8:], st
    assert new.half_tail(multiples[0], False) == [0] * 8 and new.half_tail(multiples[3], True) == [0] * 8


def test_permutation_with_the_new_layer_equals_the_oracle():
    new, _ = _models()
    rng = np.random.default_rng(183)
    states = np.concatenate([np.arange(16, dtype=np.uint32)[None], rng.integers(0, P, (1_000, 16), dtype=np.uint32)])
    want = ob.poseidon2_permute(states).reshape(-1, 16).tolist()
    for st, w in zip(states.tolist(), want):
        assert new.permute(st) == w, st
    assert want[0] == KAT_OUT
