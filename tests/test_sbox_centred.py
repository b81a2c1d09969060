"""CPU model of the lane-form S-box in centred form (PermT::pow5c and its canon_rc, recursive-stwo_amd/csrc/poseidon2.hpp).

    m  = canon_rc(t) with rc' = (rc + 2^30) mod P    = (t + rc + 2^30) mod P in [0, P - 1]   (two literal adds + v_min)
    x  = m - 2^30                                    [-2^30, 2^30 - 2], congruent to t + rc
    xx = x + x                                       [-2^31, 2^31 - 4], even: an int32
    V1 = xx * x + KP                                 v_mad_i64_i32, KP = -P * 2^32 (SGPR pair): 2x^2 - P * 2^32
    s1 = hi(V1) + (lo(V1) >> 1)  as int32            fold2(2x^2) - P in [-P, 2^29], congruent to x^2
    V2 = s1 * s1 + KN                                v_mad_i64_i32, KN = -P * 2^31: [-P * 2^31, -P]
    c4 = alignbit(hi(V2), lo(V2), 31) + (lo(V2) & P) (V2 >> 31) + (V2 & P) = fold(s1^2) - P in [-P, P - 2], congruent to x^4
    V3 = xx * c4 + KQ                                v_mad_i64_i32, KQ = P * 2^31: [2^32, 2^32 * P], even
    y  = hi(V3) + (lo(V3) >> 1)                      [0, 2P - 1], congruent to x^5

No conditional subtract after the first one: x^2 and x^4 stay signed and centred.  The last product is the one a signed S-box
has to resolve (two full-width signed operands span 2 P^2, one bit more than a 32-bit fold takes): x is centred so that 2x
is an int32, the product is even and spans 2^32 * P < 2^63, and the two-instruction fold2 ends it.

The model restates every instruction on 32- and 64-bit words (wrapping where the hardware wraps; v_mad_i64_i32 reads its
operands as int32 and its addend as int64), asserts each range on the way, and is run on the extremes of every range, on
edge and random inputs, and inside the whole permutation (the model of tests/test_partial_pairs.py with this S-box), which
must equal the oracle.  The output range is the old S-box's, so the HI bounds of the header hold as they are."""
import numpy as np

from tests import oracle_binding as ob
from tests import test_partial_pairs as tpp

P = 0x7FFFFFFF
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
CENTRE = 1 << 30
KP = (1 << 64) - (P << 32)
KN = (1 << 64) - (P << 31)
KQ = P << 31


def _i32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def _i64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def _mad_i64_i32(a, b, c):  # v_mad_i64_i32: int32 x int32 + int64, the 64-bit result word
    a, b, c = _i32(a), _i32(b), _i64(c)
    d = a * b + c
    assert -(1 << 63) <= d < 1 << 63, (a, b, c)                    # exact: no int64 overflow
    return d & M64


def _alignbit(hi, lo, sh):  # v_alignbit_b32: bits sh .. sh + 31 of hi:lo
    return ((hi << 32 | lo) >> sh) & M32


def centred(rc):
    return (rc + CENTRE) % P


def _canon_rc(t, rc):  # PermT::canon_rc<centred(rc), HI>
    c = P - centred(rc)
    return min((t - c) & M32, (t + (P - c)) & M32)


def _sbox(m, seen=None):
    """pow5c on machine words; `seen` collects every intermediate for the range checks."""
    assert 0 <= m <= P - 1
    x = _i32(m - CENTRE)                                            # v_add_u32 with a literal
    xx = _i32(x + x)                                                # v_add_u32
    V1 = _mad_i64_i32(xx, x, KP)
    s1 = _i32((V1 >> 32) + ((V1 & M32) >> 1))                       # fold2, read as a signed word
    V2 = _mad_i64_i32(s1, s1, KN)
    c4 = _i32(_alignbit(V2 >> 32, V2 & M32, 31) + (V2 & M32 & P))
    V3 = _mad_i64_i32(xx, c4, KQ)
    y = ((V3 >> 32) + ((V3 & M32) >> 1)) & M32
    if seen is not None:
        seen.update(x=x, xx=xx, V1=_i64(V1), s1=s1, V2=_i64(V2), c4=c4, V3=_i64(V3), y=y)
    return y


def _check_ranges(m):
    v = {}
    y = _sbox(m, v)
    x = v["x"]
    assert -CENTRE <= x <= CENTRE - 2 and (x - m) % P == (-CENTRE) % P, m
    assert v["xx"] == 2 * x and v["xx"] % 2 == 0, m                  # the doubling does not wrap
    assert v["V1"] == 2 * x * x - (P << 32), m                      # the addend is exact, not a wrap
    assert -P <= v["s1"] <= 1 << 29 and v["s1"] % P == x * x % P, m
    assert v["V2"] == v["s1"] ** 2 - (P << 31) and -(P << 31) <= v["V2"] <= -P, m
    assert -P <= v["c4"] <= P - 2 and v["c4"] % P == pow(x, 4, P), m
    assert v["V3"] == 2 * x * v["c4"] + (P << 31), m
    assert 0 <= v["V3"] <= P << 32 and v["V3"] % 2 == 0, m         # fold2's contract: even, below 2^63
    assert y <= 2 * P - 1, m                                        # L2, the old S-box's bound
    assert y % P == pow(x, 5, P), m
    return v


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    edge = [0, 1, 2, 3, P - 3, P - 2, P - 1, CENTRE - 2, CENTRE - 1, CENTRE, CENTRE + 1, CENTRE + 2, 1 << 15, 1 << 16,
            CENTRE - 46341, CENTRE + 46341, CENTRE - 46340, CENTRE + 46340, P // 2, P // 2 + 1]
    return edge + [int(v) for v in rng.integers(0, P, n)]


def test_bounds_proven_over_the_whole_input_range():
    """Interval bounds for every m in [0, P - 1], step by step, then the inputs that reach the ends of the intervals."""
    x_lo, x_hi = 0 - CENTRE, P - 1 - CENTRE
    assert (x_lo, x_hi) == (-(1 << 30), (1 << 30) - 2)
    xx_lo, xx_hi = 2 * x_lo, 2 * x_hi
    assert -(1 << 31) <= xx_lo and xx_hi < 1 << 31                  # 2x is an int32 because x is centred
    # V1 = 2x^2 - P * 2^32; 2x^2 <= 2^61, so fold2(2x^2) = (2x^2 >> 32) + (lo >> 1) <= 2^29 + 2^31 - 1 and s1 = that - P
    sq2_hi = 2 * max(x_lo * x_lo, x_hi * x_hi)
    assert sq2_hi == 1 << 61
    s1_lo, s1_hi = 0 - P, (sq2_hi >> 32) + (M32 >> 1) - P
    assert (s1_lo, s1_hi) == (-P, 1 << 29)
    # V2 = s1^2 - P * 2^31 <= P^2 - P * 2^31 = -P; its arithmetic shift by 31 stays in [-P, -1] and fits an int32
    sq_hi = max(s1_lo * s1_lo, s1_hi * s1_hi)
    assert sq_hi == P * P
    V2_lo, V2_hi = -(P << 31), sq_hi - (P << 31)
    assert V2_hi == -P and V2_lo >> 31 == -P and V2_hi >> 31 == -1
    # c4 = (V2 >> 31) + (V2 & P) = (s1^2 >> 31) + (s1^2 & P) - P; at s1^2 = P^2 the shift is P - 1 and the low part 1
    c4_lo, c4_hi = -P, max(((P * P) >> 31) + ((P * P) & P), (((P * P) >> 31) - 1) + P) - P
    assert (c4_lo, c4_hi) == (-P, P - 2)
    # the last product: the extremes of xx * c4 are at the corners
    corners = [a * b for a in (xx_lo, xx_hi) for b in (c4_lo, c4_hi)]
    V3_lo, V3_hi = min(corners) + (P << 31), max(corners) + (P << 31)
    assert V3_lo >= 0 and V3_hi == P << 32 and V3_hi < 1 << 63
    # fold2: hi <= P (only at V3 = P * 2^32, with lo = 0), otherwise hi <= P - 1 and lo >> 1 <= 2^31 - 1
    y_hi = max(P, P - 1 + (M32 >> 1))
    assert y_hi == 2 * P - 1                                        # the bound of the old pow5: HI_FULL / HI_PARTIAL hold
    assert tpp._model(tpp.Bound).pow5(P) == y_hi
    # the ends: m = 0 gives xx = -2^31, and s1 = -P at x = 0 (m = 2^30), where V2 = P^2 - P * 2^31
    v = _check_ranges(CENTRE)
    assert v["x"] == 0 and v["s1"] == -P and v["V2"] == -P and v["c4"] == (P * P >> 31) + 1 - P
    v = _check_ranges(0)
    assert v["xx"] == -(1 << 31)
    assert _check_ranges(P - 1)["xx"] == (1 << 31) - 4


def test_every_input_near_the_range_ends():
    """All m within 2^12 of either end of [0, P - 1] and of the values where x, s1 or c4 change sign or reach a bound."""
    worst = dict(s1_lo=P, s1_hi=-P, c4_lo=P, c4_hi=-P, V3_lo=1 << 63, V3_hi=0, y=0)
    for c in [0, P - 1, CENTRE, CENTRE - 46341, CENTRE + 46341, 1 << 16, P // 2]:
        for m in range(max(0, c - 4096), min(P - 1, c + 4096) + 1):
            v = _check_ranges(m)
            worst["s1_lo"] = min(worst["s1_lo"], v["s1"])
            worst["s1_hi"] = max(worst["s1_hi"], v["s1"])
            worst["c4_lo"] = min(worst["c4_lo"], v["c4"])
            worst["c4_hi"] = max(worst["c4_hi"], v["c4"])
            worst["V3_lo"] = min(worst["V3_lo"], v["V3"])
            worst["V3_hi"] = max(worst["V3_hi"], v["V3"])
            worst["y"] = max(worst["y"], v["y"])
    assert worst["s1_lo"] == -P and worst["s1_hi"] <= 1 << 29
    assert worst["c4_lo"] >= -P and worst["c4_hi"] <= P - 2
    assert worst["V3_lo"] >= 0 and worst["V3_hi"] <= P << 32 and worst["y"] <= 2 * P - 1


def test_congruent_to_x5_on_edge_and_random_inputs():
    for m in _inputs(200_000, 41):
        _check_ranges(m)


def test_fused_reduction_with_the_shifted_constants():
    """canon_rc<centred(rc), HI>: for every call site's constant the shifted one still leaves room for HI (the header's
    static_assert), and the reduction gives (t + rc + 2^30) mod P over the whole input range t <= P + HI."""
    hi_full, hi_partial, _ = tpp._header()
    full, partial = tpp._constants()
    sites = [(rc, hi_full) for r in (0, 1, 2, 3, 5, 6, 7) for rc in full[r]]
    sites += [(rc, hi_partial) for rc in full[4]] + [(rc, hi_partial) for rc in partial]
    assert len(sites) == 142
    rng = np.random.default_rng(42)
    for rc, hi in sites:
        assert hi < P - centred(rc), hex(rc)
        c = P - centred(rc)
        for t in [0, 1, c - 1, c, c + 1, P - 1, P, P + 1, P + hi - 1, P + hi] + [int(v) for v in rng.integers(0, P + hi + 1, 64)]:
            if 0 <= t <= P + hi:
                assert _canon_rc(t, rc) == (t + rc + CENTRE) % P, (hex(rc), t)


class Exact(tpp.Exact):
    """Concrete values, the centred S-box."""

    @staticmethod
    def pow5c(m):
        return _sbox(m)


class Bound(tpp.Bound):
    """Upper bounds: the S-box returns the largest value it can (test_bounds_proven_over_the_whole_input_range)."""

    @staticmethod
    def pow5c(m):
        assert m <= P - 1
        return 2 * P - 1


class CentredModel(tpp.Model):
    """The permutation model of tests/test_partial_pairs.py with the centred S-box: every canon_rc reduces with the
    shifted constant (and the model asserts HI against it) and pow5 takes its canonical output m."""

    def canon_rc(self, t, rc, hi, site):
        return super().canon_rc(t, centred(rc), hi, site)

    def pow5(self, m):
        return self.ar.pow5c(m)


def _model(ar):
    return CentredModel(ar, tpp._constants(), *tpp._header())


def test_header_states_the_centred_sbox():
    """The kernel's S-box is the one modelled here: the three addends, the centring, canon_rc with the shifted constants at
    every call site, and one v_min per S-box (canon_rc's)."""
    src = open(tpp.HDR).read()
    assert "KN = 0 - ((uint64_t)P << 31), KQ = (uint64_t)P << 31" in src and "CENTRE = 1u << 30" in src
    body = src[src.index("uint32_t pow5c(uint32_t m, const SboxK& k)"):]
    body = body[:body.index("\n    }\n")]
    assert "m - CENTRE" in body and "mad64s(xx, x, k.kp)" in body and "sqr64s(s1, k.kn)" in body
    assert "mad64s(xx, (int32_t)c4, k.kq)" in body and "__builtin_amdgcn_alignbit(" in body
    assert "canon(" not in body and "min(" not in body
    rounds = src[src.index("void sbox_full(const uint64_t* V"):src.index("// Everything up to and including the S-box layer")]
    assert rounds.count("pow5c(canon_rc<centred(") == 5 and "pow5(" not in rounds


def test_bounds_hold_for_every_input():
    """The permutation on upper bounds with this S-box: the asserts of the model hold for the largest value every step can
    produce, and every canon_rc input stays within the header's HI for its shifted constant."""
    m = _model(Bound)
    assert m.permute([P] * 16) == [P] * 16
    hi_full, hi_partial, _ = tpp._header()
    assert m.rc_inputs["full"] <= hi_full and m.rc_inputs["partial"] <= hi_partial
    assert m.rc_inputs["full4"] <= (1 << 18) + 64


def test_permutation_with_centred_sbox_equals_the_oracle():
    m = _model(Exact)
    rng = np.random.default_rng(43)
    states = [list(range(16)), [0] * 16, [P] * 16, [P - 1] * 16, [P if i % 2 else 0 for i in range(16)]]
    states += [[int(v) for v in rng.integers(0, P, 16)] for _ in range(60)]
    for st in states:
        want = ob.poseidon2_permute(np.array([v % P for v in st], dtype=np.uint32)).reshape(-1).tolist()
        assert m.permute(st) == want, st
