"""CPU model of the lane-form permutation's paired partial rounds (PermT::partial_pair, recursive-stwo_amd/csrc/poseidon2.hpp).

Two consecutive partial rounds R, R + 1 are computed in one pass: with S the sum of round R and d_i = 2^(i+1),
    S'    = u0' + sum_{i>=1} d_i s_i + 15 S
    s_i'' = (d_i^2 mod P) s_i + d_i S + S'
so round R's words 1..15 are never formed.  The words then leave a pair weakly reduced up to about P + 2^30, and the
arithmetic relies on bounds that this file proves: the model restates the kernel's fast path statement by statement in
Python integers (doubled 64-bit accumulators, fold2, the fused round-constant reduction canon_rc with the real constants)
and is run twice — on concrete states, where it must give the oracle's permutation, and on UPPER BOUNDS, where every step
is monotone, so the asserts hold for every input the kernel can see:
  * every v_mad_u64_u32 result is below 2^64 (and even: every multiplier or multiplicand is);
  * every fold2 input V is even and below 2^63 (V = 2v, v < 2^62), so hi32(V) + (lo32(V) >> 1) fits 32 bits;
  * every canon_rc input is <= P + HI, with HI < P - rc for that call site's constant.
The schedule (which rounds are single, which paired) and the HI bounds are read from the header itself."""
import ctypes
import os
import re

import numpy as np

from tests import oracle_binding as ob

P = 0x7FFFFFFF
M32 = 0xFFFFFFFF
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recursive-stwo_amd", "csrc", "poseidon2.hpp")


def _constants():
    ob.lib.rsvo_round_constants.restype = ctypes.POINTER(ctypes.c_uint32)
    ob.lib.rsvo_round_constants.argtypes = [ctypes.c_int]
    first = [ob.lib.rsvo_round_constants(0)[i] for i in range(64)]
    partial = [ob.lib.rsvo_round_constants(1)[i] for i in range(14)]
    last = [ob.lib.rsvo_round_constants(2)[i] for i in range(64)]
    return [first[16 * r:16 * r + 16] for r in range(4)] + [last[16 * r:16 * r + 16] for r in range(4)], partial


def _header():
    """(HI_FULL, HI_PARTIAL, schedule) as poseidon2.hpp states them; schedule = [("round" | "pair", R), ...]."""
    src = open(HDR).read()
    m = re.search(r"HI_FULL = (\d+), HI_PARTIAL = 1u << (\d+);", src)
    body = re.search(r"void poseidon2_rounds\(.*?\n    }\n", src, re.S).group(0)
    sched = [(k, int(r)) for k, r in re.findall(r"partial_(round|pair)<(\d+)>\(s,", body)]
    return int(m.group(1)), 1 << int(m.group(2)), sched


class Exact:
    """Concrete values: the kernel's arithmetic."""

    @staticmethod
    def fold2(V):
        assert V % 2 == 0 and V < 1 << 63, hex(V)
        return (V >> 32) + ((V & M32) >> 1)

    @staticmethod
    def canon(t):
        assert t <= 2 * P, hex(t)
        return min(t, (t - P) & M32)

    @staticmethod
    def canon_rc(t, rc, hi):
        c = P - rc
        return min((t - c) & M32, (t + (P - c)) & M32)

    @staticmethod
    def even(a, b):
        assert a % 2 == 0 or b % 2 == 0


class Bound:
    """Upper bounds: every operation of the model is monotone in its inputs once fold2 and the reductions are replaced by
    the largest value they can return."""

    @staticmethod
    def fold2(V):
        assert V < 1 << 63, hex(V)
        return (V >> 32) + (M32 >> 1)

    @staticmethod
    def canon(t):
        assert t <= 2 * P, hex(t)
        return P

    @staticmethod
    def canon_rc(t, rc, hi):
        return P - 1

    @staticmethod
    def even(a, b):
        pass


class Model:
    def __init__(self, ar, consts, hi_full, hi_partial, sched):
        self.ar, (self.full, self.partial) = ar, consts
        self.hi_full, self.hi_partial, self.sched = hi_full, hi_partial, sched
        self.rc_inputs = {}  # call site -> largest canon_rc input seen

    # ---- 64-bit accumulator instructions
    def mad(self, a, b, c=0):  # v_mad_u64_u32
        assert 0 <= a <= M32 and 0 <= b <= M32 and 0 <= c < 1 << 64
        self.ar.even(a, b)
        d = a * b + c
        assert d < 1 << 64, hex(d)
        return d

    def add64(self, a, b, sh=0):  # v_lshl_add_u64
        d = (a << sh) + b
        assert d < 1 << 64
        return d

    def fold2(self, V):
        r = self.ar.fold2(V)
        assert r <= M32
        return r

    def canon_rc(self, t, rc, hi, site):
        assert hi < P - rc, (site, hex(rc))
        assert t <= P + hi, (site, hex(t))
        self.rc_inputs[site] = max(self.rc_inputs.get(site, 0), t - P)
        return self.ar.canon_rc(t, rc, hi)

    def pow5(self, x):
        assert x <= P
        xx = 2 * x
        c2 = self.ar.canon(self.fold2(self.mad(xx, x)))
        c4 = self.ar.canon(self.fold2(self.mad(2 * c2, c2)))
        return self.fold2(self.mad(xx, c4))

    # ---- linear layers
    def mds16_2x(self, s):
        V = [0] * 16
        for g in range(4):
            x0, x1, x2, x3 = s[4 * g:4 * g + 4]
            T0 = self.mad(x0, 2, self.mad(x1, 2))
            T1 = self.mad(x2, 2, self.mad(x3, 2))
            T2, T3 = self.mad(x1, 4, T1), self.mad(x3, 4, T0)
            T4, T5 = self.add64(T1, T3, 2), self.add64(T0, T2, 2)
            V[4 * g:4 * g + 4] = [self.add64(T3, T5), T5, self.add64(T2, T4), T4]
        for j in range(4):
            col = self.add64(self.add64(V[j], V[j + 4]), self.add64(V[j + 8], V[j + 12]))
            for g in range(4):
                V[4 * g + j] = self.add64(V[4 * g + j], col)
        return V

    def sbox_full(self, V, r):
        return [self.pow5(self.canon_rc(self.fold2(V[i]), self.full[r][i], self.hi_full, "full")) for i in range(16)]

    def partial_round(self, s, r):
        s = list(s)
        u0 = self.pow5(self.canon_rc(s[0], self.partial[r], self.hi_partial, "partial"))
        a, b = self.mad(u0, 2), self.mad(s[1], 2)
        for i in range(2, 16, 2):
            a, b = self.mad(s[i], 2, a), self.mad(s[i + 1], 2, b)
        sum2 = self.add64(a, b)
        s[0] = self.fold2(self.mad(u0, 6, sum2))
        for i in range(1, 16):
            s[i] = self.fold2(self.mad(s[i], 1 << (i + 2), sum2))
        return s

    def partial_pair(self, s, r):
        s = list(s)
        u0 = self.pow5(self.canon_rc(s[0], self.partial[r], self.hi_partial, "partial"))
        a, b = self.mad(u0, 2), self.mad(s[1], 2)
        for i in range(2, 16, 2):
            a, b = self.mad(s[i], 2, a), self.mad(s[i + 1], 2, b)
        sum2 = self.add64(a, b)
        s0, sf = self.fold2(self.mad(u0, 6, sum2)), self.fold2(sum2)
        u0 = self.pow5(self.canon_rc(s0, self.partial[r + 1], self.hi_partial, "partial"))
        kd = [6] + [1 << (i + 2) for i in range(1, 16)]
        kq = [0] + [2 * pow(2, 2 * i + 2, P) for i in range(1, 16)]
        a, b = self.mad(u0, 2), self.mad(s[1], kd[1])
        for i in range(2, 16, 2):
            a, b = self.mad(s[i], kd[i], a), self.mad(s[i + 1], kd[i + 1], b)
        a = self.mad(sf, 30, a)
        sum2 = self.add64(a, b)
        out = [self.fold2(self.mad(u0, 6, sum2))]
        for i in range(1, 16):
            out.append(self.fold2(self.mad(s[i], kq[i], self.mad(sf, kd[i], sum2))))
        return out

    def partial_section(self, s):
        for kind, r in self.sched:
            s = self.partial_pair(s, r) if kind == "pair" else self.partial_round(s, r)
        return s

    def permute(self, s):
        V = self.mds16_2x(s)
        for r in range(4):
            V = self.mds16_2x(self.sbox_full(V, r))
        s = self.partial_section([self.fold2(v) for v in V])
        s = [self.pow5(self.canon_rc(s[i], self.full[4][i], self.hi_partial, "full4")) for i in range(16)]
        V = self.mds16_2x(s)
        for r in range(5, 8):
            V = self.mds16_2x(self.sbox_full(V, r))
        out = []
        for v in V:
            t = self.fold2(v)
            assert t <= P + self.hi_full
            out.append(self.ar.canon(t))
        return out


def _model(ar):
    return Model(ar, _constants(), *_header())


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
    hi_full, hi_partial, sched = _header()
    assert _rounds(sched) == list(range(14))
    assert sched[-1][0] == "round", "the words handed to sbox_full4 must come from a single round"
    assert sum(kind == "pair" for kind, _ in sched) == 6


def test_bounds_hold_for_every_input():
    """The model on upper bounds: the asserts of Model hold for the largest value every step can produce, from a canonical
    input state (the permutation's contract) — the proof behind the kernel's static_asserts and comments."""
    m = _model(Bound)
    out = m.permute([P] * 16)
    assert out == [P] * 16
    hi_full, hi_partial, _ = _header()
    # the bounds poseidon2.hpp states at its call sites
    assert m.rc_inputs["full"] <= hi_full and m.rc_inputs["partial"] <= hi_partial
    assert m.rc_inputs["full4"] <= (1 << 18) + 64                  # <= P + 2^18 + 2^6 after the last, single, round
    # every word entering the partial rounds: the fold of a full-round layer
    V = m.mds16_2x([Bound.fold2(2 * P * P)] * 16)
    entry = [Bound.fold2(v) for v in V]
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
    m = _model(Exact)
    rng = np.random.default_rng(21)
    states = [list(range(16)), [0] * 16, [P] * 16, [P - 1] * 16, [P if i % 2 else 0 for i in range(16)]]
    states += [[int(v) for v in rng.integers(0, P, 16)] for _ in range(60)]
    for st in states:
        want = ob.poseidon2_permute(np.array([v % P for v in st], dtype=np.uint32)).reshape(-1).tolist()
        assert m.permute(st) == want, st


def test_partial_section_at_its_extremes():
    """The partial rounds alone, from the states the full rounds can hand them (every word up to P + HI_FULL), and each
    pair alone from the largest words the schedule can hand it: the result is congruent to the specification's rounds."""
    m = _model(Exact)
    hi_full, _, sched = _header()
    top = P + hi_full
    rng = np.random.default_rng(22)
    states = [[top] * 16, [0] * 16, [P] * 16, [top if i % 2 else 0 for i in range(16)], [0] + [top] * 15, [top] + [0] * 15]
    states += [[int(v) for v in rng.integers(0, top + 1, 16)] for _ in range(100)]
    for st in states:
        got = m.partial_section(st)
        assert [v % P for v in got] == _partial_ref(st, m.partial, _rounds(sched)), st
    # each pair on its own: every word at the bound the steps before it can produce (word 0 at the S-box's limit)
    b = _model(Bound)
    s = [top] * 16
    for kind, r in sched:
        if kind == "pair":
            for st in ([P + m.hi_partial] + s[1:], s[:1] + [v - 1 for v in s[1:]], [0] + s[1:]):
                got = m.partial_pair(st, r)
                assert [v % P for v in got] == _partial_ref(st, m.partial, [r, r + 1]), (r, st)
        s = b.partial_pair(s, r) if kind == "pair" else b.partial_round(s, r)
