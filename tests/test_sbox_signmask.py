"""The S-box's entry on machine words (PermT::centre_rc, recursive-stwo_amd/csrc/poseidon2.hpp; the model is tests/perm_model.py).

With rc' = (rc + 2^30) mod P and c = P - rc', the centred representative of t + rc is x = ((t + rc') mod P) - 2^30, in
[-2^30, 2^30 - 2].  centre_rc selects the reduction by the sign of a = t - c.  a is an int32 in [-c, P + HI - c] (it does not
wrap: c > HI, and the upper end is HI + rc' < P), and the two addends a - 2^30 and a + P - 2^30 take are bit-complements of
each other:

    a  = t - c                   literal add, wrapping on 32 bits
    sg = a >> 31  (arithmetic)   v_ashrrev_i32: 0 or 0xFFFFFFFF
    q  = sg ^ 0xC0000000         0xC0000000 = -2^30 for a >= 0, 0x3FFFFFFF = P - 2^30 for a < 0
    x  = a + q                   wrapping on 32 bits, read as an int32

The reference is the same select by an unsigned minimum, min_u32(t - c, t - c + P) - 2^30 (perm_model.vmin_form).  This file
proves x bit-identical to it at every call site of the permutation: at the edges of t for that site's constant and HI, on
random (t, site) pairs, and inside the whole permutation model, which checks every entry on the way and must equal the oracle."""
import numpy as np

from tests import perm_model as pm
from tests.perm_model import CENTRE, M32, P


def test_the_two_addends_are_complements():
    assert (0 - CENTRE) & M32 == 0xC0000000 and P - CENTRE == 0x3FFFFFFF
    assert 0xC0000000 ^ M32 == 0x3FFFFFFF
    assert pm.ashr31(0x80000000) == M32 and pm.ashr31(0x7FFFFFFF) == 0 and pm.ashr31(0) == 0


def test_equal_to_the_vmin_form_at_every_call_site_edge():
    for rc, hi in pm.sites():
        c = P - pm.centred(rc)
        assert hi < c                                                # the header's static_assert: c > HI
        assert P + hi - c <= 0x7FFFFFFF                              # and its second one: the upper end of a is an int32
        for t in (0, 1, c - 1, c, c + 1, P - 1, P, P + hi):
            pm.check_entry(t, rc, hi)
        assert pm.centre_rc(c - 1, rc)[1] == -1 and pm.centre_rc(c, rc)[1] == 0 and pm.centre_rc(0, rc)[1] == -c


def test_equal_to_the_vmin_form_on_random_inputs():
    sites = pm.sites()
    rng = np.random.default_rng(161)
    which = rng.integers(0, len(sites), 200_000)
    frac = rng.random(200_000)
    for k, f in zip(which.tolist(), frac.tolist()):
        rc, hi = sites[k]
        pm.check_entry(int(f * (P + hi + 1)), rc, hi)


def test_difference_never_leaves_int32_over_the_whole_range():
    """Interval proof: t in [0, P + HI] gives a in [-c, P + HI - c]; both ends are int32 values for every site."""
    for rc, hi in pm.sites():
        c = P - pm.centred(rc)
        assert -(1 << 31) <= -c and P + hi - c < 1 << 31
        assert pm.centre_rc(0, rc)[1] == -c and pm.centre_rc(P + hi, rc)[1] == P + hi - c


def test_permutation_with_signmask_entry_equals_the_oracle():
    """Every S-box entry of the run goes through perm_model.check_entry: compared with the v_min form on the way."""
    assert pm.Exact.entry is pm.check_entry
    pm.assert_equals_oracle(162, extra=([1] * 16,))


def test_bounds_hold_with_the_signmask_entry():
    """On upper bounds the model's asserts hold and every centre_rc input stays within the header's HI."""
    pm.assert_bounds_hold()


def test_header_states_the_signmask_entry():
    """The kernel's entry is the one modelled here: both asserts, the arithmetic shift, the literal, and all five call sites
    of the permutation on centre_rc, handing x straight to pow5c."""
    src = open(pm.HDR).read()
    body = src[src.index("int32_t centre_rc(uint32_t t)"):]
    body = body[:body.index("\n    }\n")]
    assert "static_assert(HI < P - RC" in body and "static_assert((uint64_t)P + HI - c <= 0x7FFFFFFFull" in body
    assert "constexpr uint32_t c = P - RC;" in body and "(int32_t)(t - c)" in body
    assert "(a >> 31) ^ 0xC0000000u" in body and "(uint32_t)a + q" in body
    assert "min(" not in body
    assert "uint32_t pow5c(int32_t x, const SboxK& k) {" in src
    rounds = src[src.index("void sbox_full(const uint64_t* V"):src.index("// Everything up to and including the S-box layer")]
    assert rounds.count("pow5c(centre_rc<centred(") == 5 and rounds.count("pow5c(") == 5     # no other arm
