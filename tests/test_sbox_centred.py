"""The lane-form S-box on machine words (PermT::pow5c, recursive-stwo_amd/csrc/poseidon2.hpp; the model is tests/perm_model.py).

    x                                                [-2^30, 2^30 - 2], the centred representative of t + rc (centre_rc)
    xx = x + x                                       [-2^31, 2^31 - 4], even: an int32
    V1 = xx * x + KP                                 v_mad_i64_i32, KP = -P * 2^32 (SGPR pair): 2x^2 - P * 2^32
    s1 = hi(V1) + (lo(V1) >> 1)  as int32            fold2(2x^2) - P in [-P, 2^29], congruent to x^2
    V2 = s1 * s1 + KN                                v_mad_i64_i32, KN = -P * 2^31: [-P * 2^31, -P]
    c4 = alignbit(hi(V2), lo(V2), 31) + (lo(V2) & P) (V2 >> 31) + (V2 & P) = fold(s1^2) - P in [-P, P - 2], congruent to x^4
    V3 = xx * c4 + KQ                                v_mad_i64_i32, KQ = P * 2^31: [0, 2^32 * P], even
    y  = hi(V3) + (lo(V3) >> 1)                      [0, 2P - 1], congruent to x^5

No conditional subtract: x^2 and x^4 stay signed and centred.  The last product is the one a signed S-box has to resolve (two
full-width signed operands span 2 P^2, one bit more than a 32-bit fold takes): x is centred so that 2x is an int32, the
product is even and spans 2^32 * P < 2^63, and the two-instruction fold2 ends it.

The model wraps where the hardware wraps (v_mad_i64_i32 reads its operands as int32 and its addend as int64).  This file
asserts each range on the way: by interval arithmetic, on the extremes of every range, on edge and random inputs, and inside
the whole permutation, which must equal the oracle.  Inputs are listed as m = x + 2^30 in [0, P - 1]."""
import numpy as np

from tests import perm_model as pm
from tests.perm_model import CENTRE, M32, P


def _check_ranges(m):
    v = {}
    y = pm.pow5c(m - CENTRE, v)
    x = v["x"]
    assert -CENTRE <= x <= CENTRE - 2, m
    assert v["xx"] == 2 * x and v["xx"] % 2 == 0, m                  # the doubling does not wrap
    assert v["V1"] == 2 * x * x - (P << 32), m                      # the addend is exact, not a wrap
    assert -P <= v["s1"] <= 1 << 29 and v["s1"] % P == x * x % P, m
    assert v["V2"] == v["s1"] ** 2 - (P << 31) and -(P << 31) <= v["V2"] <= -P, m
    assert -P <= v["c4"] <= P - 2 and v["c4"] % P == pow(x, 4, P), m
    assert v["V3"] == 2 * x * v["c4"] + (P << 31), m
    assert 0 <= v["V3"] <= P << 32 and v["V3"] % 2 == 0, m         # fold2's contract: even, below 2^63
    assert y <= 2 * P - 1, m                                        # L2: what HI_FULL / HI_PARTIAL are derived from
    assert y % P == pow(x, 5, P), m
    return v


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    edge = [0, 1, 2, 3, P - 3, P - 2, P - 1, CENTRE - 2, CENTRE - 1, CENTRE, CENTRE + 1, CENTRE + 2, 1 << 15, 1 << 16,
            CENTRE - 46341, CENTRE + 46341, CENTRE - 46340, CENTRE + 46340, P // 2, P // 2 + 1]
    return edge + [int(v) for v in rng.integers(0, P, n)]


def test_bounds_proven_over_the_whole_input_range():
    """Interval bounds for every x in [-2^30, 2^30 - 2], step by step, then the inputs that reach the ends of the intervals."""
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
    assert y_hi == 2 * P - 1
    assert pm.Bound.pow5c(x_hi) == y_hi                             # the value the upper-bound run of the permutation uses
    # the ends: x = -2^30 gives xx = -2^31, and s1 = -P at x = 0, where V2 = P^2 - P * 2^31
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
    """centre_rc<centred(rc), HI>: for every call site's constant the shifted one still leaves room for HI (the header's
    static_assert), and the reduction gives (t + rc + 2^30) mod P, less 2^30, over the whole input range t <= P + HI."""
    rng = np.random.default_rng(42)
    for rc, hi in pm.sites():
        assert hi < P - pm.centred(rc), hex(rc)
        c = P - pm.centred(rc)
        for t in [0, 1, c - 1, c, c + 1, P - 1, P, P + 1, P + hi - 1, P + hi] + [int(v) for v in rng.integers(0, P + hi + 1, 64)]:
            if 0 <= t <= P + hi:
                assert pm.centre_rc(t, rc)[0] == (t + rc + CENTRE) % P - CENTRE, (hex(rc), t)


def test_header_states_the_centred_sbox():
    """The kernel's S-box is the one modelled here: the three addends, the centring of the round constants, one pow5c with
    the three signed products and the alignbit fold and no conditional subtract, entered through centre_rc at all five call
    sites; the forms it replaced are gone from the header."""
    src = open(pm.HDR).read()
    assert "KP = 0 - ((uint64_t)P << 32)" in src
    assert "KN = 0 - ((uint64_t)P << 31), KQ = (uint64_t)P << 31" in src and "CENTRE = 1u << 30" in src
    assert src.count("uint32_t pow5c(") == 1
    body = src[src.index("uint32_t pow5c(int32_t x, const SboxK& k)"):]
    body = body[:body.index("\n    }\n")]
    assert "dbl32((uint32_t)x)" in body and "mad64s(xx, x, k.kp)" in body and "sqr64s(s1, k.kn)" in body
    assert "mad64s(xx, (int32_t)c4, k.kq)" in body and "__builtin_amdgcn_alignbit(" in body
    assert "canon(" not in body and "min(" not in body and "CENTRE" not in body
    rounds = src[src.index("void sbox_full(const uint64_t* V"):src.index("// Everything up to and including the S-box layer")]
    assert rounds.count("pow5c(centre_rc<centred(") == 5 and rounds.count("pow5c(") == 5 and "pow5(" not in rounds
    perm_t = src[src.index("struct PermT {"):src.index("// (tools/perm_lab.hip, k_permute: the paced form)")]
    assert "canon_rc" not in perm_t and "RSV_SBOX_VMIN" not in src and " pow5(" not in perm_t and "canon(" not in perm_t


def test_bounds_hold_for_every_input():
    """The permutation on upper bounds with the S-box at its largest output: the asserts of the model hold for the largest
    value every step can produce, and every centre_rc input stays within the header's HI for its shifted constant."""
    pm.assert_bounds_hold()


def test_permutation_with_centred_sbox_equals_the_oracle():
    pm.assert_equals_oracle(43)
