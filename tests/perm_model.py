"""Machine-word model of the lane-form permutation (PermT, recursive-stwo_amd/csrc/poseidon2.hpp), for the CPU tests.

The model restates the kernel's fast path statement by statement in Python integers, wrapping where the hardware wraps and
asserting where the code relies on a value not wrapping:

    fold2      V = 2v -> hi32(V) + (lo32(V) >> 1)
    centre_rc  the S-box's entry: t <= P + HI and a round constant -> the centred x congruent to t + rc, by sign mask
    pow5c      x -> x^5 on signed words, three v_mad_i64_i32 with the addends KP, KN, KQ
    Model      the 64-bit accumulator instructions, the linear layers, the single and paired partial rounds, the permutation

Model runs over one of two arithmetics: Exact (concrete values: the kernel's words, which must give the oracle's
permutation) and Bound (upper bounds: every operation of the model is monotone in its inputs once fold2, the entry and the
S-box are replaced by the largest value they can return, so an assert that holds on the bounds holds for every input the
kernel can see).  The asserts are the proof behind the header's static_asserts and range comments:
  * every v_mad_u64_u32 result is below 2^64 (and even: every multiplier or multiplicand is);
  * every fold2 input V is even and below 2^63 (V = 2v, v < 2^62), so the fold fits 32 bits;
  * every centre_rc input is <= P + HI, with HI < c and P + HI - c an int32 for that call site's constant.
HI_FULL, HI_PARTIAL and the schedule of single and paired partial rounds are read from the header itself."""
import ctypes
import os
import re

from tests import oracle_binding as ob

P = 0x7FFFFFFF
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
CENTRE = 1 << 30
KP = (1 << 64) - (P << 32)  # the S-box's addends as 64-bit words: -P * 2^32, -P * 2^31, P * 2^31
KN = (1 << 64) - (P << 31)
KQ = P << 31
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recursive-stwo_amd", "csrc", "poseidon2.hpp")


# ---- what the tests read from outside: the oracle's round constants and the header's bounds and schedule
def constants():
    """(full[8][16], partial[14]) from the oracle's table"""
    ob.lib.rsvo_round_constants.restype = ctypes.POINTER(ctypes.c_uint32)
    ob.lib.rsvo_round_constants.argtypes = [ctypes.c_int]
    first = [ob.lib.rsvo_round_constants(0)[i] for i in range(64)]
    partial = [ob.lib.rsvo_round_constants(1)[i] for i in range(14)]
    last = [ob.lib.rsvo_round_constants(2)[i] for i in range(64)]
    return [first[16 * r:16 * r + 16] for r in range(4)] + [last[16 * r:16 * r + 16] for r in range(4)], partial


def header():
    """(HI_FULL, HI_PARTIAL, schedule) as poseidon2.hpp states them; schedule = [("round" | "pair", R), ...]."""
    src = open(HDR).read()
    m = re.search(r"HI_FULL = (\d+), HI_PARTIAL = 1u << (\d+);", src)
    body = re.search(r"void poseidon2_rounds\(.*?\n    }\n", src, re.S).group(0)
    sched = [(k, int(r)) for k, r in re.findall(r"partial_(round|pair)<(\d+)>\(s,", body)]
    return int(m.group(1)), 1 << int(m.group(2)), sched


def sites():
    """(round constant, HI) of the 142 S-box call sites"""
    hi_full, hi_partial, _ = header()
    full, partial = constants()
    out = [(rc, hi_full) for r in (0, 1, 2, 3, 5, 6, 7) for rc in full[r]]
    out += [(rc, hi_partial) for rc in full[4]] + [(rc, hi_partial) for rc in partial]
    assert len(out) == 142
    return out


# ---- machine words
def i32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def i64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def mad_i64_i32(a, b, c):  # v_mad_i64_i32: int32 x int32 + int64, the 64-bit result word
    a, b, c = i32(a), i32(b), i64(c)
    d = a * b + c
    assert -(1 << 63) <= d < 1 << 63, (a, b, c)                    # exact: no int64 overflow
    return d & M64


def alignbit(hi, lo, sh):  # v_alignbit_b32: bits sh .. sh + 31 of hi:lo
    return ((hi << 32 | lo) >> sh) & M32


def ashr31(v):  # v_ashrrev_i32 by 31 on a 32-bit word
    return M32 if (v >> 31) & 1 else 0


def fold2(V):
    assert V % 2 == 0 and 0 <= V < 1 << 63, hex(V)
    return (V >> 32) + ((V & M32) >> 1)


# ---- the S-box's entry
def centred(rc):
    return (rc + CENTRE) % P


def centre_rc(t, rc):
    """PermT::centre_rc<centred(rc), HI> on machine words: (x as an int32, a as an int32, the unwrapped t - c)."""
    c = P - centred(rc)
    a = (t - c) & M32                                               # literal add, wrapping on 32 bits
    q = ashr31(a) ^ 0xC0000000                                      # -2^30 for a >= 0, P - 2^30 for a < 0
    x = (a + q) & M32
    return i32(x), i32(a), t - c


def vmin_form(t, rc):
    """Reference arithmetic, not in the header: the same select by an unsigned minimum, min(t - c, t - c + P) - 2^30 on
    32-bit words."""
    c = P - centred(rc)
    return (min((t - c) & M32, (t + (P - c)) & M32) - CENTRE) & M32


def check_entry(t, rc, hi):
    """centre_rc at one call site's constant and HI, with everything the header claims about it; returns x."""
    x, a, exact = centre_rc(t, rc)
    assert a == exact, (hex(rc), t)                                  # t - c never leaves the int32 range
    assert -(P - centred(rc)) <= a <= hi + centred(rc) < P, (hex(rc), t)
    assert x & M32 == vmin_form(t, rc), (hex(rc), t)                 # bit-identical to the v_min form
    assert x == (t + rc + CENTRE) % P - CENTRE, (hex(rc), t)
    assert -CENTRE <= x <= CENTRE - 2 and (x - t - rc) % P == 0, (hex(rc), t)
    return x


# ---- the S-box
def pow5c(x, seen=None):
    """PermT::pow5c on machine words; `seen` collects every intermediate for the range checks."""
    assert -CENTRE <= x <= CENTRE - 2
    xx = i32(x + x)                                                 # v_add_u32
    V1 = mad_i64_i32(xx, x, KP)
    s1 = i32((V1 >> 32) + ((V1 & M32) >> 1))                        # fold2, read as a signed word
    V2 = mad_i64_i32(s1, s1, KN)
    c4 = i32(alignbit(V2 >> 32, V2 & M32, 31) + (V2 & M32 & P))
    V3 = mad_i64_i32(xx, c4, KQ)
    y = ((V3 >> 32) + ((V3 & M32) >> 1)) & M32
    if seen is not None:
        seen.update(x=x, xx=xx, V1=i64(V1), s1=s1, V2=i64(V2), c4=c4, V3=i64(V3), y=y)
    return y


# ---- the two arithmetics
class Exact:
    """Concrete values: the kernel's arithmetic."""
    fold2 = staticmethod(fold2)
    entry = staticmethod(check_entry)
    pow5c = staticmethod(pow5c)

    @staticmethod
    def canon(t):
        assert t <= 2 * P, hex(t)
        return min(t, (t - P) & M32)

    @staticmethod
    def even(a, b):
        assert a % 2 == 0 or b % 2 == 0


class Bound:
    """Upper bounds: fold2 returns the largest fold of anything up to V, the S-box the largest value it can return
    (tests/test_sbox_centred.py proves 2P - 1) whatever its input."""

    @staticmethod
    def fold2(V):
        assert V < 1 << 63, hex(V)
        return (V >> 32) + (M32 >> 1)

    @staticmethod
    def entry(t, rc, hi):
        return CENTRE - 2

    @staticmethod
    def pow5c(x):
        assert -CENTRE <= x <= CENTRE - 2
        return 2 * P - 1

    @staticmethod
    def canon(t):
        assert t <= 2 * P, hex(t)
        return P

    @staticmethod
    def even(a, b):
        pass


class Model:
    def __init__(self, ar, consts, hi_full, hi_partial, sched):
        self.ar, (self.full, self.partial) = ar, consts
        self.hi_full, self.hi_partial, self.sched = hi_full, hi_partial, sched
        self.rc_inputs = {}  # call site -> largest centre_rc input seen, less P

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

    def sbox(self, t, rc, hi, site):  # pow5c(centre_rc<centred(rc), hi>(t), k)
        assert hi < P - centred(rc), (site, hex(rc))                 # the header's two static_asserts
        assert P + hi - (P - centred(rc)) <= 0x7FFFFFFF, (site, hex(rc))
        assert t <= P + hi, (site, hex(t))
        self.rc_inputs[site] = max(self.rc_inputs.get(site, 0), t - P)
        return self.ar.pow5c(self.ar.entry(t, rc, hi))

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
        return [self.sbox(self.fold2(V[i]), self.full[r][i], self.hi_full, "full") for i in range(16)]

    def partial_round(self, s, r):
        s = list(s)
        u0 = self.sbox(s[0], self.partial[r], self.hi_partial, "partial")
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
        u0 = self.sbox(s[0], self.partial[r], self.hi_partial, "partial")
        a, b = self.mad(u0, 2), self.mad(s[1], 2)
        for i in range(2, 16, 2):
            a, b = self.mad(s[i], 2, a), self.mad(s[i + 1], 2, b)
        sum2 = self.add64(a, b)
        s0, sf = self.fold2(self.mad(u0, 6, sum2)), self.fold2(sum2)
        u0 = self.sbox(s0, self.partial[r + 1], self.hi_partial, "partial")
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
        s = [self.sbox(s[i], self.full[4][i], self.hi_partial, "full4") for i in range(16)]
        V = self.mds16_2x(s)
        for r in range(5, 8):
            V = self.mds16_2x(self.sbox_full(V, r))
        out = []
        for v in V:
            t = self.fold2(v)
            assert t <= P + self.hi_full
            out.append(self.ar.canon(t))
        return out


def model(ar):
    return Model(ar, constants(), *header())


def assert_equals_oracle(seed, extra=()):
    """The model on concrete values gives the oracle's permutation: the special states and 60 random ones."""
    import numpy as np
    m = model(Exact)
    rng = np.random.default_rng(seed)
    states = [list(range(16)), [0] * 16, [P] * 16, [P - 1] * 16, [P if i % 2 else 0 for i in range(16)], *extra]
    states += [[int(v) for v in rng.integers(0, P, 16)] for _ in range(60)]
    for st in states:
        want = ob.poseidon2_permute(np.array([v % P for v in st], dtype=np.uint32)).reshape(-1).tolist()
        assert m.permute(st) == want, st


def assert_bounds_hold():
    """The model on upper bounds from a canonical input state (the permutation's contract): its asserts hold for the
    largest value every step can produce, and every centre_rc input stays within the header's HI.  Returns the model."""
    m = model(Bound)
    assert m.permute([P] * 16) == [P] * 16
    hi_full, hi_partial, _ = header()
    assert m.rc_inputs["full"] <= hi_full and m.rc_inputs["partial"] <= hi_partial
    assert m.rc_inputs["full4"] <= (1 << 18) + 64                  # <= P + 2^18 + 2^6 after the last, single, round
    return m
