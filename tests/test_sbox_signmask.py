"""CPU model of the S-box entry without its v_min (PermT::centre_rc, recursive-stwo_amd/csrc/poseidon2.hpp).

canon_rc reduces t + rc' (rc' = (rc + 2^30) mod P, c = P - rc') with two literal adds and a v_min, and pow5c subtracts 2^30:

    m = min_u32(t - c, t - c + P)        x = m - 2^30 in [-2^30, 2^30 - 2]

centre_rc selects by the sign of a = t - c instead.  a is an int32 in [-c, P + HI - c] (it does not wrap: c > HI, and the upper
end is HI + rc' < P), and the two addends a - 2^30 and a + P - 2^30 take are bit-complements of each other:

    a  = t - c                   literal add, wrapping on 32 bits
    sg = a >> 31  (arithmetic)   v_ashrrev_i32: 0 or 0xFFFFFFFF
    q  = sg ^ 0xC0000000         0xC0000000 = -2^30 for a >= 0, 0x3FFFFFFF = P - 2^30 for a < 0
    x  = a + q                   wrapping on 32 bits, read as an int32

The model restates the four instructions on 32-bit machine words and proves x equal to the v_min form at every call site of
the permutation: at the edges of t for that site's constant and HI, on random (t, site) pairs, and inside the whole permutation
model (tests/test_sbox_centred.py with this entry), which must equal the oracle."""
import re

import numpy as np

from tests import oracle_binding as ob
from tests import test_partial_pairs as tpp
from tests import test_sbox_centred as tsc

P = 0x7FFFFFFF
M32 = 0xFFFFFFFF
CENTRE = 1 << 30


def _ashr31(v):  # v_ashrrev_i32 by 31 on a 32-bit word
    return M32 if (v >> 31) & 1 else 0


def _centre_rc(t, rc):
    """PermT::centre_rc<centred(rc), HI> on machine words: (x as an int32, a as an int32, the unwrapped t - c)."""
    c = P - tsc.centred(rc)
    a = (t - c) & M32
    sg = _ashr31(a)
    q = sg ^ 0xC0000000
    x = (a + q) & M32
    return tsc._i32(x), tsc._i32(a), t - c


def _vmin_form(t, rc):
    """today's entry: canon_rc's v_min, then pow5c's centring subtract, as a 32-bit word"""
    return (tsc._canon_rc(t, rc) - CENTRE) & M32


def _sites():
    hi_full, hi_partial, _ = tpp._header()
    full, partial = tpp._constants()
    sites = [(rc, hi_full) for r in (0, 1, 2, 3, 5, 6, 7) for rc in full[r]]
    sites += [(rc, hi_partial) for rc in full[4]] + [(rc, hi_partial) for rc in partial]
    assert len(sites) == 142
    return sites


def _check(t, rc, hi):
    x, a, exact = _centre_rc(t, rc)
    assert a == exact, (hex(rc), t)                                  # t - c never leaves the int32 range
    assert -(P - tsc.centred(rc)) <= a <= hi + tsc.centred(rc) < P, (hex(rc), t)
    assert x & M32 == _vmin_form(t, rc), (hex(rc), t)                # bit-identical to the v_min form
    assert -CENTRE <= x <= CENTRE - 2 and (x - t - rc) % P == 0, (hex(rc), t)
    return x


def test_the_two_addends_are_complements():
    assert (0 - CENTRE) & M32 == 0xC0000000 and P - CENTRE == 0x3FFFFFFF
    assert 0xC0000000 ^ M32 == 0x3FFFFFFF
    assert _ashr31(0x80000000) == M32 and _ashr31(0x7FFFFFFF) == 0 and _ashr31(0) == 0


def test_equal_to_the_vmin_form_at_every_call_site_edge():
    for rc, hi in _sites():
        c = P - tsc.centred(rc)
        assert hi < c                                                # the header's static_assert: c > HI
        assert P + hi - c <= 0x7FFFFFFF                              # and its second one: the upper end of a is an int32
        for t in (0, 1, c - 1, c, c + 1, P - 1, P, P + hi):
            _check(t, rc, hi)
        assert _centre_rc(c - 1, rc)[1] == -1 and _centre_rc(c, rc)[1] == 0 and _centre_rc(0, rc)[1] == -c


def test_equal_to_the_vmin_form_on_random_inputs():
    sites = _sites()
    rng = np.random.default_rng(161)
    which = rng.integers(0, len(sites), 200_000)
    frac = rng.random(200_000)
    for k, f in zip(which.tolist(), frac.tolist()):
        rc, hi = sites[k]
        _check(int(f * (P + hi + 1)), rc, hi)


def test_difference_never_leaves_int32_over_the_whole_range():
    """Interval proof: t in [0, P + HI] gives a in [-c, P + HI - c]; both ends are int32 values for every site."""
    for rc, hi in _sites():
        c = P - tsc.centred(rc)
        assert -(1 << 31) <= -c and P + hi - c < 1 << 31
        assert _centre_rc(0, rc)[1] == -c and _centre_rc(P + hi, rc)[1] == P + hi - c


class SignMaskModel(tsc.CentredModel):
    """The permutation model of tests/test_sbox_centred.py entered through centre_rc: the S-box takes x, handed on as
    m = x + 2^30 (pow5c's x overload), and every entry is compared with the v_min form on the way."""

    def canon_rc(self, t, rc, hi, site):
        m = super().canon_rc(t, rc, hi, site)
        if self.ar is Exact:
            x = _check(t, rc, hi)
            assert x + CENTRE == m, (site, hex(rc), t)
            return x + CENTRE
        return m


class Exact(tsc.Exact):
    pass


def _model(ar):
    return SignMaskModel(ar, tpp._constants(), *tpp._header())


def test_permutation_with_signmask_entry_equals_the_oracle():
    m = _model(Exact)
    rng = np.random.default_rng(162)
    states = [list(range(16)), [0] * 16, [P] * 16, [P - 1] * 16, [P if i % 2 else 0 for i in range(16)], [1] * 16]
    states += [[int(v) for v in rng.integers(0, P, 16)] for _ in range(60)]
    for st in states:
        want = ob.poseidon2_permute(np.array([v % P for v in st], dtype=np.uint32)).reshape(-1).tolist()
        assert m.permute(st) == want, st


def test_bounds_hold_with_the_signmask_entry():
    """On upper bounds the entry returns what canon_rc returns (the largest m), so the HI bounds are those of the centred
    form: the model's asserts hold and every centre_rc input stays within the header's HI."""
    m = _model(tsc.Bound)
    assert m.permute([P] * 16) == [P] * 16
    hi_full, hi_partial, _ = tpp._header()
    assert m.rc_inputs["full"] <= hi_full and m.rc_inputs["partial"] <= hi_partial


def test_header_states_the_signmask_entry():
    """The kernel's entry is the one modelled here: both asserts, the arithmetic shift, the literal, the x overload of pow5c,
    and all five call sites of the permutation on centre_rc."""
    src = open(tpp.HDR).read()
    body = src[src.index("int32_t centre_rc(uint32_t t)"):]
    body = body[:body.index("\n    }\n")]
    assert "static_assert(HI < P - RC" in body and "static_assert((uint64_t)P + HI - c <= 0x7FFFFFFFull" in body
    assert "constexpr uint32_t c = P - RC;" in body and "(int32_t)(t - c)" in body
    assert "(a >> 31) ^ 0xC0000000u" in body and "(uint32_t)a + q" in body
    assert "min(" not in body
    assert "uint32_t pow5c(int32_t x, const SboxK& k) { return pow5c((uint32_t)x + CENTRE, k); }" in src
    assert re.search(r"#ifndef RSV_SBOX_VMIN\n\s*static constexpr bool CENTRE_RC = true;", src)
    rounds = src[src.index("void sbox_full(const uint64_t* V"):src.index("// Everything up to and including the S-box layer")]
    assert rounds.count("CENTRE_RC ? pow5c(centre_rc<centred(") == 5
