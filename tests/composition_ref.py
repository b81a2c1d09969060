"""Test helper (numpy, no device): tree 3 of the next proof, the composition polynomial, restated over tests/commit_ref.py
(circle interpolation and evaluation) and the oracle's eval_composition (tests/oracle_binding.py oods_eval).  It holds no
second implementation of the constraints: every column is extended to CanonicCoset(clb).circle_domain(), clb =
max(lp + 2, lq + 3), the 142-value sample vector of each row is built (the tree 3 slots are unused by the accumulator),
oods_eval gives every row's accumulator at once, and the four coordinates are interpolated, cut at the middle and
evaluated on the domain 2^(clb - 1).  The previous row of a position is found through the points' circle-group indices,
not through an index formula.  tests/test_composition_host.py pins these conventions to the reference;
tests/test_composition_gpu.py compares the device against this helper."""
import numpy as np

from tests import commit_ref as C
from tests import oracle_binding as ob

P = C.P


def clb_of(lp, lq):
    return max(lp + 2, lq + 3)


def domain_indices(N, r=None):
    """k[r]: the point at storage position r of CanonicCoset(N).circle_domain() is k[r] * GEN (k mod 2^31); every position
    of the domain by default."""
    i = C.bit_reverse(np.arange(1 << N, dtype=np.int64) if r is None else np.asarray(r, dtype=np.int64), N)
    half = 1 << (N - 1)
    k = (1 << (30 - N)) + (i & (half - 1)) * (1 << (32 - N))
    return np.where(i >= half, -k, k) & ((1 << 31) - 1)


def prev_positions(N, log):
    """The storage position of the point minus the step of CanonicCoset(log), for every position of the domain 2^N."""
    k = domain_indices(N)
    order = np.argsort(k)
    want = (k - (1 << (31 - log))) & ((1 << 31) - 1)
    pos = order[np.searchsorted(k[order], want)]
    assert np.array_equal(k[pos], want)
    return pos


def sample_vectors(plonk, poseidon, plonk_prev, poseidon_prev):
    """plonk = (pre [10, n], trace [12, n], interaction [8, n]) and poseidon = ([40, n], [48, n], [8, n]): M31 mask values
    of n points; *_prev [4, n]: the cumulative columns 4..7 at the previous-row points -> uint32[n, 142, 4] in the proof's
    order of sampled values (first words; the tree 3 slots zero)."""
    n = np.asarray(plonk[0]).shape[1]
    s = np.zeros((n, 142), np.int64)
    s[:, 0:10], s[:, 10:50] = np.asarray(plonk[0]).T, np.asarray(poseidon[0]).T
    s[:, 50:62], s[:, 62:110] = np.asarray(plonk[1]).T, np.asarray(poseidon[1]).T
    for off, inter, prev in ((110, plonk[2], plonk_prev), (122, poseidon[2], poseidon_prev)):
        s[:, off:off + 4] = np.asarray(inter)[:4].T
        s[:, off + 4:off + 12:2] = np.asarray(prev).T
        s[:, off + 5:off + 12:2] = np.asarray(inter)[4:].T
    out = np.zeros((n, 142, 4), np.uint32)
    out[:, :, 0] = s % P
    return out


def accumulator(samples, lp, lq, sums, draws, xs):
    """oods_eval's acc for every sample vector at the points with x = (xs[i], 0, 0, 0): uint32[n, 4].  sums: [2][4], draws:
    z, alpha, random_coeff (12 words)."""
    n = samples.shape[0]
    par = np.zeros((n, 26), np.uint32)
    par[:, 0], par[:, 1] = lp, lq
    par[:, 2:10] = np.asarray(sums, dtype=np.int64).reshape(8) % P
    par[:, 10:22] = np.asarray(draws, dtype=np.int64).reshape(12) % P
    par[:, 22] = xs
    return ob.oods_eval(samples, par)[:, :4]


def composition(plonk, poseidon, lp, lq, sums, draws):
    """One proof: -> (columns int64[8, 2^L3], coefficients int64[8, 2^L3]) of tree 3."""
    clb = clb_of(lp, lq)
    L3 = clb - 1
    ep = [C.lde(np.asarray(c, dtype=np.int64) % P, lp, clb - lp) for c in plonk]
    eq = [C.lde(np.asarray(c, dtype=np.int64) % P, lq, clb - lq) for c in poseidon]
    samples = sample_vectors(ep, eq, ep[2][4:, prev_positions(clb, lp)], eq[2][4:, prev_positions(clb, lq)])
    acc = accumulator(samples, lp, lq, sums, draws, C.gen_mul(domain_indices(clb))[0])
    co = C.interpolate(acc.T.astype(np.int64), clb)
    halves = np.concatenate([co[:, :1 << L3], co[:, 1 << L3:]])
    return C.evaluate(halves, L3, L3), halves


def eval_m31(coeffs, log, x, y):
    """CirclePoly::eval_at_point of coefficient rows int64[k, 2^log] at the M31 point (x, y) -> int64[k]."""
    folds = [y % P, x % P]
    for _ in range(2, log):
        folds.append((2 * folds[-1] * folds[-1] - 1) % P)
    v = np.asarray(coeffs, dtype=np.int64) % P
    for f in folds[:log]:
        v = v.reshape(v.shape[0], -1, 2)
        v = (v[:, :, 0] + v[:, :, 1] * f) % P
    return v[:, 0]


# The shapes of tests/test_composition_gpu.py::test_composition_bit_for_bit
SHAPES = [  # (lp, lq, n, mask, shared preprocessed columns)
    (4, 3, 2, None, False),       # clb = 6 from the Plonk term
    (3, 5, 3, [1, 0, 1], False),  # clb = 8 from the Poseidon term, Plonk over-extended by 2^5; one proof masked
    (6, 6, 2, None, True),        # preprocessed columns shared by every proof (stride 0)
    (11, 10, 2, None, False),     # clb = 13: just past the 4 096-point switch between the LDS and the global FFT stages
]
