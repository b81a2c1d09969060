"""The lane-form permutation's linear layers and paired partial rounds (PermT::partial_pair, recursive-stwo_amd/csrc/poseidon2.hpp)
on the machine-word model of tests/perm_model.py.

Two consecutive partial rounds R, R + 1 are computed in one pass: with S the sum of round R and d_i = 2^(i+1),
    S'    = u0' + sum_{i>=1} d_i s_i + 15 S
    s_i'' = (d_i^2 mod P) s_i + d_i S + S'
so round R's words 1..15 are never formed.  The words then leave a pair weakly reduced up to about P + 2^30, and the
arithmetic relies on bounds that this file proves by running the model twice: on concrete states, where it must give the
oracle's permutation, and on UPPER BOUNDS, where every step is monotone, so the model's asserts hold for every input the
kernel can see."""
import numpy as np

from tests import perm_model as pm
from tests.perm_model import P


def _partial_ref(s, partial, rounds):
    """the partial rounds of the specification, mod P"""
    s = [v % P for v in s]
    for r in rounds:
        s[0] = pow((s[0] + partial[r]) % P, 5, P)
        tot = sum(s) % P
        s = [(3 * s[0] + tot) % P] + [((1 << (i + 1)) * s[i] + tot) % P for i in range(1, 16)]
    return s


def _rounds(sched):
    return [r for kind, r in sched for r in ((r, r + 1) if kind == "pair" else (r,))]


def test_schedule_covers_the_fourteen_partial_rounds():
    hi_full, hi_partial, sched = pm.header()
    assert _rounds(sched) == list(range(14))
    assert sched[-1][0] == "round", "the words handed to sbox_full4 must come from a single round"
    assert sum(kind == "pair" for kind, _ in sched) == 6


def test_bounds_hold_for_every_input():
    """The model on upper bounds: the asserts of Model hold for the largest value every step can produce, from a canonical
    input state (the permutation's contract) — the proof behind the kernel's static_asserts and comments."""
    m = pm.assert_bounds_hold()                                     # the bounds poseidon2.hpp states at its call sites
    hi_full, hi_partial, _ = pm.header()
    # every word entering the partial rounds: the fold of a full-round layer
    V = m.mds16_2x([pm.Bound.fold2(2 * P * P)] * 16)
    entry = [pm.Bound.fold2(v) for v in V]
    assert max(entry) <= P + hi_full
    # the pairs' outputs: near 2^32 for the words with multiplier 2^29 and 2^31, still inside 32 bits and within what the
    # next pair's 2^31 * s_14 < 2^63 allows
    s = entry
    for kind, r in m.sched:
        s = m.partial_pair(s, r) if kind == "pair" else m.partial_round(s, r)
        if kind == "pair":
            assert max(s) < (1 << 32) - (1 << 24) and s[0] <= P + hi_partial
        else:
            assert max(s) <= P + (1 << 18) + (1 << 6)


def test_kernel_arithmetic_equals_the_oracle():
    pm.assert_equals_oracle(21)


def test_kernel_arithmetic_equals_the_oracle_on_a_second_seed():
    pm.assert_equals_oracle(32)


def test_partial_section_at_its_extremes():
    """The partial rounds alone, from the states the full rounds can hand them (every word up to P + HI_FULL), and each
    pair alone from the largest words the schedule can hand it: the result is congruent to the specification's rounds."""
    m = pm.model(pm.Exact)
    hi_full, _, sched = pm.header()
    top = P + hi_full
    rng = np.random.default_rng(22)
    states = [[top] * 16, [0] * 16, [P] * 16, [top if i % 2 else 0 for i in range(16)], [0] + [top] * 15, [top] + [0] * 15]
    states += [[int(v) for v in rng.integers(0, top + 1, 16)] for _ in range(100)]
    for st in states:
        got = m.partial_section(st)
        assert [v % P for v in got] == _partial_ref(st, m.partial, _rounds(sched)), st
    # each pair on its own: every word at the bound the steps before it can produce (word 0 at the S-box's limit)
    b = pm.model(pm.Bound)
    s = [top] * 16
    for kind, r in sched:
        if kind == "pair":
            for st in ([P + m.hi_partial] + s[1:], s[:1] + [v - 1 for v in s[1:]], [0] + s[1:]):
                got = m.partial_pair(st, r)
                assert [v % P for v in got] == _partial_ref(st, m.partial, [r, r + 1]), (r, st)
        s = b.partial_pair(s, r) if kind == "pair" else b.partial_round(s, r)
