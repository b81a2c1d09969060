"""CPU model of the lane-form S-box with the signed middle square (PermT::pow5, recursive-stwo_amd/csrc/poseidon2.hpp).

    xx = 2x                                          x in C = [0, P]
    V1 = xx * x + K  mod 2^64                        K = 2^64 - P * 2^32 (v_mad_u64_u32, SGPR-pair addend, carry dropped)
    s1 = hi(V1) + (lo(V1) >> 1)  as int32            = t1 - P with t1 = fold2(2x^2): in [-P, P - 1], congruent to x^2
    V2 = s1 * s1                                     v_mad_i64_i32: [0, P^2]
    t2 = alignbit(hi(V2), lo(V2), 31) + (lo(V2) & P) = (V2 >> 31) + (V2 & P): [0, 2P - 1]
    c4 = min(t2, t2 - P)                             C, congruent to x^4
    y  = fold2(xx * c4)                              2x * c4 < 2^63: y in L2, congruent to x^5

The model restates every instruction on 32- and 64-bit words (wrapping where the hardware wraps), asserts each range on
the way, and is run on the extremes of every range, on edge and random inputs, and inside the whole permutation (the model
of tests/test_partial_pairs.py with this pow5), which must equal the oracle."""
import numpy as np

from tests import oracle_binding as ob
from tests import test_partial_pairs as tpp

P = 0x7FFFFFFF
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
K = (1 << 64) - (P << 32)


def _i32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def _alignbit(hi, lo, sh):  # v_alignbit_b32: bits sh .. sh + 31 of hi:lo
    return ((hi << 32 | lo) >> sh) & M32


def _sbox(x, seen=None):
    """The kernel's S-box on machine words; `seen` collects every intermediate for the range checks."""
    assert 0 <= x <= P
    xx = (x + x) & M32
    V1 = (xx * x + K) & M64                                         # v_mad_u64_u32: the carry-out is dropped
    s1 = _i32((V1 >> 32) + ((V1 & M32) >> 1))                       # fold2, read as a signed word
    V2 = (s1 * s1) & M64                                            # v_mad_i64_i32, no addend
    t2 = (_alignbit(V2 >> 32, V2 & M32, 31) + (V2 & M32 & P)) & M32
    c4 = min(t2, (t2 - P) & M32)
    prod = xx * c4                                                  # v_mad_u64_u32, no addend
    assert prod < 1 << 63
    y = (prod >> 32) + ((prod & M32) >> 1)
    if seen is not None:
        seen.update(xx=xx, s1=s1, V2=V2, t2=t2, c4=c4, prod=prod, y=y, t1=(2 * x * x >> 32) + ((2 * x * x & M32) >> 1))
    return y


def _check_ranges(x):
    v = {}
    y = _sbox(x, v)
    assert v["t1"] <= 2 * P - 1 and v["s1"] == v["t1"] - P, x
    assert -P <= v["s1"] <= P - 1, x
    assert v["s1"] % P == x * x % P, x
    assert 0 <= v["V2"] <= P * P and v["V2"] == v["s1"] * v["s1"], x
    assert v["t2"] <= 2 * P - 1, x
    assert v["c4"] <= P and v["c4"] % P == pow(x, 4, P), x
    assert v["prod"] < 1 << 63, x
    assert y <= 2 * P and y < 1 << 32, x                           # L2, as before the signed square
    assert y % P == pow(x, 5, P), x
    return v


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    edge = [0, 1, 2, 3, P - 2, P - 1, P, 1 << 15, (1 << 15) + 1, 1 << 16, (1 << 16) - 1, 46340, 46341, 1 << 30,
            (1 << 30) - 1, (1 << 30) + 1, P // 2, P // 2 + 1]
    return edge + [int(v) for v in rng.integers(0, P + 1, n)]


def test_bounds_proven_over_the_whole_input_range():
    """Interval bounds for every x in C, step by step (each step is monotone in the quantities bounded), then the inputs
    that reach the ends of the intervals."""
    # t1 = fold2(2x^2) = (x^2 >> 31) + (x^2 & P), x^2 <= P^2
    t1_hi = ((P * P) >> 31) + P
    assert t1_hi == 2 * P - 1
    # the addend K takes P * 2^32 off the product and leaves its low word alone, so the fold comes out P lower (mod 2^32);
    # t1 - P lies in [-P, P - 1], inside int32, so the signed reading of the wrapped word is exact
    s1_lo, s1_hi = 0 - P, t1_hi - P
    assert (s1_lo, s1_hi) == (-P, P - 1) and -(1 << 31) <= s1_lo and s1_hi < 1 << 31
    V2_hi = max(s1_lo * s1_lo, s1_hi * s1_hi)
    assert V2_hi == P * P and V2_hi < 1 << 62                       # v_mad_i64_i32 of two int32: exact
    t2_hi = (V2_hi >> 31) + P                                       # V2 >> 31 <= P - 1 for every V2 <= P^2
    assert t2_hi == 2 * P - 1 and t2_hi < 1 << 32
    c4_hi = P                                                       # t2 < P: t2; t2 >= P: t2 - P <= P - 1
    prod_hi = 2 * P * c4_hi
    assert prod_hi < 1 << 63
    y_hi = (prod_hi >> 32) + (M32 >> 1)
    assert y_hi <= 2 * P and y_hi < 1 << 32                         # L2, the bound the old pow5's last fold gave
    # the old pow5's last step is the same multiply and fold, so the permutation's upper-bound run holds as it is
    m = tpp._model(tpp.Bound)
    assert m.pow5(P) == y_hi
    # the ends: x = 0 gives t1 = 0, s1 = -P and V2 = P^2; x = P (congruent to 0) gives t1 = (P - 1) + 1 and s1 = 0
    v = _check_ranges(0)
    assert v["s1"] == -P and v["V2"] == P * P
    assert _check_ranges(P)["s1"] == 0


def test_every_input_near_the_range_ends():
    """All x within 2^12 of either end of C and of the values where s1 or t2 change sign or wrap."""
    worst = dict(s1_lo=P, s1_hi=-P, t2=0, V2=0)
    centres = [0, P, 46341, 1 << 16, 1 << 30, P // 2]
    for c in centres:
        for x in range(max(0, c - 4096), min(P, c + 4096) + 1):
            v = _check_ranges(x)
            worst["s1_lo"] = min(worst["s1_lo"], v["s1"])
            worst["s1_hi"] = max(worst["s1_hi"], v["s1"])
            worst["t2"] = max(worst["t2"], v["t2"])
            worst["V2"] = max(worst["V2"], v["V2"])
    assert worst["s1_lo"] == -P and worst["V2"] == P * P
    assert worst["s1_hi"] <= P - 1 and worst["t2"] <= 2 * P - 1


def test_congruent_to_x5_on_edge_and_random_inputs():
    for x in _inputs(200_000, 31):
        _check_ranges(x)


class SignedModel(tpp.Model):
    """The permutation model of tests/test_partial_pairs.py with this pow5."""

    def pow5(self, x):
        return _sbox(x)


def test_header_states_the_signed_square():
    """The kernel's pow5 is the one modelled here: the SGPR-pair addend 2^64 - P * 2^32, the signed square and the
    alignbit fold, and no canon() before the square."""
    src = open(tpp.HDR).read()
    assert "0 - ((uint64_t)P << 32)" in src
    body = src[src.index("uint32_t pow5(uint32_t x, uint64_t kp)"):]
    body = body[:body.index("\n    }\n")]
    assert "sqr64s(" in body and "mad64(xx, x, kp, 0)" in body and "__builtin_amdgcn_alignbit(" in body
    assert body.count("canon(") == 1 and body.count("mul64(") == 1


def test_permutation_with_signed_sbox_equals_the_oracle():
    m = SignedModel(tpp.Exact, tpp._constants(), *tpp._header())
    rng = np.random.default_rng(32)
    states = [list(range(16)), [0] * 16, [P] * 16, [P - 1] * 16, [P if i % 2 else 0 for i in range(16)]]
    states += [[int(v) for v in rng.integers(0, P, 16)] for _ in range(60)]
    for st in states:
        want = ob.poseidon2_permute(np.array([v % P for v in st], dtype=np.uint32)).reshape(-1).tolist()
        assert m.permute(st) == want, st
