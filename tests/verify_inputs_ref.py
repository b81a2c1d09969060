"""What the tests of per-proof public inputs share (no test lives here): a Python-integer model of the statement's share of
the logup balance, sum_i 1 / (v_i + (idx_i mod P) alpha - z), written from csrc/field.hpp (q_inv through c_inv and m_inv =
a^(P-2), so that the inverse of 0 is 0); a model of the kernel's batched inversion (csrc/k_pi_sum.hpp: input k on lane k mod
64, eight denominators per lane per inversion, a zero left out of the running product); and a variant of
tests/user_circuit_ref.py's S1 with many public inputs, built with the oracle's constraint system."""
import numpy as np

from oracle.recursion_circuit import cs as C
from oracle.recursion_circuit import gadgets as G
from tests import user_circuit_ref as U

P = 0x7FFFFFFF
LANES, CHUNK = 64, 8


# ---------------------------------------------------------------- field.hpp in Python integers
def m_inv(a):
    return pow(a, P - 2, P)  # 0 -> 0


def c_mul(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def c_mul_r(x):  # x * (2 + i)
    return ((2 * x[0] - x[1]) % P, (2 * x[1] + x[0]) % P)


def c_inv(x):
    n = m_inv((x[0] * x[0] + x[1] * x[1]) % P)
    return (x[0] * n % P, (-x[1]) % P * n % P)


def q_add(x, y):
    return tuple((a + b) % P for a, b in zip(x, y))


def q_sub(x, y):
    return tuple((a - b) % P for a, b in zip(x, y))


def q_mul(x, y):
    xa, xb, ya, yb = x[:2], x[2:], y[:2], y[2:]
    ac, bd = c_mul(xa, ya), c_mul(xb, yb)
    r = c_mul_r(bd)
    ad, bc = c_mul(xa, yb), c_mul(xb, ya)
    return ((ac[0] + r[0]) % P, (ac[1] + r[1]) % P, (ad[0] + bc[0]) % P, (ad[1] + bc[1]) % P)


def q_inv(x):
    xa, xb = x[:2], x[2:]
    aa, bb = c_mul(xa, xa), c_mul_r(c_mul(xb, xb))
    den = c_inv(((aa[0] - bb[0]) % P, (aa[1] - bb[1]) % P))
    return c_mul(xa, den) + c_mul(((-xb[0]) % P, (-xb[1]) % P), den)


ZERO, ONE = (0, 0, 0, 0), (1, 0, 0, 0)


# ---------------------------------------------------------------- the sum
def denominators(records, z, alpha):
    """records: rows (idx, v0, v1, v2, v3) of one proof -> (the denominators, bad).  A value word not below P counts as 0
    and sets bad; so does a word of z or alpha; idx is taken mod P."""
    bad = False

    def canon(w):
        nonlocal bad
        w = int(w)
        if w >= P:
            bad = True
            return 0
        return w
    z, alpha = tuple(canon(w) for w in z), tuple(canon(w) for w in alpha)
    out = []
    for r in records:
        v = tuple(canon(w) for w in r[1:5])
        k = int(r[0]) % P
        out.append(q_sub(q_add(v, tuple(a * k % P for a in alpha)), z))
    return out, bad


def sum_per_term(dens):
    """The loop of k_oods: one q_inv per term, the inverse of a zero denominator being what q_inv gives (0)."""
    s = ZERO
    for d in dens:
        s = q_add(s, q_inv(d))
    return s


def sum_batched(dens, lanes=LANES, chunk=CHUNK):
    """The kernel's order: term k on lane k mod lanes; a lane inverts `chunk` denominators at a time through one q_inv of
    their running product, a zero denominator left out of the product and adding nothing."""
    total = ZERO
    for lane in range(min(lanes, len(dens))):
        mine = dens[lane::lanes]
        for c0 in range(0, len(mine), chunk):
            part = mine[c0:c0 + chunk]
            run, before = ONE, []
            for d in part:
                before.append(run)
                if d != ZERO:
                    run = q_mul(run, d)
            inv = q_inv(run)
            for d, b in zip(reversed(part), reversed(before)):
                if d != ZERO:
                    total = q_add(total, q_mul(inv, b))
                    inv = q_mul(inv, d)
    return total


def model(records, z, alpha):
    """-> (sum as a list of four words, bad) for one proof: what rsv_public_input_sum_dev must write."""
    dens, bad = denominators(records, z, alpha)
    return list(sum_per_term(dens)), int(bad)


def value_for_zero(idx, z, alpha):
    """The value v with v + (idx mod P) alpha - z = 0."""
    k = int(idx) % P
    return q_sub(tuple(int(w) for w in z), tuple(int(a) * k % P for a in alpha))


def records_of(inputs):
    """[(idx, (v0..v3)), ...] -> uint32[n_pi, 5]."""
    return np.array([[k] + [int(w) for w in v] for k, v in inputs], dtype=np.uint32).reshape(-1, 5)


# ---------------------------------------------------------------- S1 with many public inputs
def build_many(n_public, first=11, seed=1, bit=1):
    """tests/user_circuit_ref.py's S1 with num_input = n_public (the three constants and n_public - 3 public inputs
    `first`, `first` + 1, ...: M31 values, as new_qm31(PublicInput) enforces); every public input is read by the circuit
    (their sum takes the place of S1's one input)."""
    assert n_public >= 4
    G.PERMUTE = U.permute
    c = C.ConstraintSystem()
    rnd = np.random.default_rng(seed)
    q = lambda: tuple(int(x) for x in rnd.integers(0, P, 4))
    pubs = []
    for k in range(n_public - 3):                              # first of all: the public inputs are variables 1 .. num_input
        v = ((first + k) % P, 0, 0, 0)
        pubs.append(C.Var(c, v, c.new_qm31(v, C.PUBLIC), 4))
    x = pubs[0]
    for p in pubs[1:]:
        x = C.add(x, p)
    a = C.qm31_witness(c, q())
    s = C.add(x, a)
    m = C.mul(s, a)
    k = C.mul_constant(m, 12345)
    w = C.m31_witness(c, int(rnd.integers(0, P)))
    k = C.add(k, C.mul(w, C.m31_constant(c, 4242)))
    k = C.mul(k, C.qm31_constant(c, (5, 6, 7, 8)))
    one = C.m31_witness(c, 1)
    b = C.m31_witness(c, bit)
    witness_ops = [(c.num_plonk_rows(), b.variable, U.OP_CONSTANT)]
    sel = C.Var(c, U.OP_CONSTANT * bit % P, c.mul_constant(b.variable, U.OP_CONSTANT if bit else 0), 1)
    k = C.add(k, sel)
    h1 = G.half_witness(c, [int(v) for v in rnd.integers(0, P, 8)])
    h2 = G.half_from_qm31(m, k)
    l1, r1 = G.permute(h1, h2, False, True)
    _, r2 = G.permute(l1, r1, True, False)
    l3, _ = G.permute(r2, G.half_zero(c), False, True, is_swap=(1, one.variable))
    l4, r4 = G.permute(l3, G.half_zero(c), False, False)
    y = C.add(l4.to_qm31()[0], x)
    y = C.mul(y, r4.to_qm31()[1])
    l5, r5 = G.permute(G.half_from_qm31(y, a), G.half_single_use(c, [int(v) for v in rnd.integers(0, P, 8)]), True, True)
    G.permute(l5, r5, True, True)
    built = U.Built(c, witness_ops)
    assert built.num_input == n_public and len(built.inputs) == n_public
    return built
