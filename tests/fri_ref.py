"""Test helper (numpy, no device): the commit phase of FRI of the next proof, restated from the verifier's formulas
(oracle/rsv_oracle.c: group_line_coeffs, row_quotient, the folds of verify_one, run_transcript) over whole columns instead
of queried positions.  QM31 arrays are int64 of shape (4, n) (tests/interaction_ref.py); the domain points come from the
circle-group indices of tests/composition_ref.py, the layer trees from the oracle's hash_node (tests/commit_ref.py
merkle_root), the channel from its half_permute (commit_ref.Channel).  tests/test_fri_host.py pins these conventions to the
reference; tests/test_fri_gpu.py compares the device against this helper."""
import numpy as np

from tests import commit_ref as C
from tests import composition_ref as K
from tests import interaction_ref as R
from tests.chain_harness import masked_past_64

P = C.P


def qs(v):
    """A QM31 4-sequence as a (4, 1) array."""
    return np.array([int(x) % P for x in v], dtype=np.int64).reshape(4, 1)


def cm(c0, c1):
    """A CM31 array pair embedded in QM31."""
    c0, c1 = np.broadcast_arrays(np.asarray(c0, dtype=np.int64) % P, np.asarray(c1, dtype=np.int64) % P)
    z = np.zeros_like(c0)
    return np.stack([c0, c1, z, z])


def domain_xy(N, pos=None):
    """(x, y) of CanonicCoset(N).circle_domain() at the storage positions pos (all by default)."""
    return C.gen_mul(K.domain_indices(N, pos))


def line_x(l, k=None):
    """x of half_odds(l).at(bit_reverse(2k, l)) for the pairs k of a line layer of log size l (all 2^(l-1) by default):
    the point of position 4k of the circle domain 2^(l+1)."""
    k = np.arange(1 << (l - 1), dtype=np.int64) if k is None else np.asarray(k, dtype=np.int64)
    return domain_xy(l + 1, 4 * k)[0]


def quotient_consts(batches, after):
    """batches: [(point ((x0..x3), (y0..y3)), [(column, value 4-tuple)])] in batch order -> [(point, columns, c (4, k), sum a,
    sum b)], the power of `after` running from -2u through every batch (group_line_coeffs)."""
    w, step = qs((0, 0, P - 2, 0)), qs(after)
    out = []
    for point, terms in batches:
        py = qs(point[1])
        y0, y1 = cm(py[0], py[1]), cm(py[2], py[3])
        sa, sb, cs = np.zeros((4, 1), np.int64), np.zeros((4, 1), np.int64), []
        for _, v in terms:
            v = qs(v)
            v0, v1 = cm(v[0], v[1]), cm(v[2], v[3])
            sa = R.q_add(sa, R.q_mul(w, v1))
            sb = R.q_add(sb, R.q_mul(w, R.q_sub(R.q_mul(v0, y1), R.q_mul(v1, y0))))
            cs.append(R.q_mul(w, y1))
            w = R.q_mul(w, step)
        out.append((point, [c for c, _ in terms], np.concatenate(cs, axis=1) if cs else np.zeros((4, 0), np.int64), sa, sb))
    return out


def row_quotient(rows, consts, x, y):
    """rows int64[n_cols, n]: the columns' values at n positions with domain points (x[i], y[i]) -> QM31 (4, n)
    (row_quotient)."""
    rows = np.asarray(rows, dtype=np.int64) % P
    x, y = np.asarray(x, dtype=np.int64) % P, np.asarray(y, dtype=np.int64) % P
    acc = np.zeros((4, rows.shape[1]), np.int64)
    for point, cols, c, sa, sb in consts:
        if not cols:
            continue
        num = np.zeros_like(acc)
        for j, col in enumerate(cols):
            num = R.q_add(num, R.q_mul_m(c[:, j:j + 1], rows[col][None, :]))
        num = R.q_sub(num, R.q_add(R.q_mul_m(sa, y[None, :]), sb))
        px, py = qs(point[0]), qs(point[1])
        prx, pix, pry, piy = cm(px[0], px[1]), cm(px[2], px[3]), cm(py[0], py[1]), cm(py[2], py[3])
        den = R.q_sub(R.q_mul(R.q_sub(prx, cm(x, 0)), piy), R.q_mul(R.q_sub(pry, cm(y, 0)), pix))
        acc = R.q_add(acc, R.q_mul(num, R.q_inv(den)))
    return acc


def fold_pairs(f0, f1, alpha, w):
    """(f0 + f1) + alpha (f0 - f1) / w for QM31 arrays f0, f1 and M31 array w."""
    return R.q_add(R.q_add(f0, f1), R.q_mul(R.q_mul_m(R.q_sub(f0, f1), C._m_inv(np.asarray(w, dtype=np.int64) % P)[None, :]), qs(alpha)))


def fold_circle(col, l, alpha):
    """A column (4, 2^l) on the circle domain -> (4, 2^(l-1)): pairs (2k, 2k + 1) with the y of position 2k."""
    col = np.asarray(col, dtype=np.int64) % P
    return fold_pairs(col[:, 0::2], col[:, 1::2], alpha, domain_xy(l, 2 * np.arange(1 << (l - 1), dtype=np.int64))[1])


def fold_line(ev, l, alpha):
    ev = np.asarray(ev, dtype=np.int64) % P
    return fold_pairs(ev[:, 0::2], ev[:, 1::2], alpha, line_x(l))


def line_interpolate(ev, L):
    """A line evaluation (4, 2^L), bit-reversed storage -> coefficients in degree order: coefficient j multiplies the
    product of pi^m(x) over the set bits m of j."""
    v = np.asarray(ev, dtype=np.int64) % P
    for m in range(L):
        # layer m pairs positions p, p + 2^m; the twiddle is pi^m of the pair's x: layer 0's of the line of size L - m
        v = v.reshape(4, 1 << (L - 1 - m), 2, 1 << m)
        a, b = v[:, :, 0, :], v[:, :, 1, :]
        w = C._m_inv(line_x(L - m))
        v = np.stack([(a + b) % P, (a - b) % P * w[None, :, None] % P], axis=2)
    return v.reshape(4, 1 << L) * pow(2, (31 - L) % 31, P) % P


def line_order(coeffs, log_n):
    """Degree order -> the order rsv_line_eval reads (index bit-reversed over log_n bits), and back."""
    return np.asarray(coeffs)[:, C.bit_reverse(np.arange(1 << log_n, dtype=np.int64), log_n)]


def layer_root(layers, ob):
    """{log size: QM31 column (4, 2^log)} -> the root of the tree over them, four M31 columns each."""
    return C.merkle_root(layers, ob)


def mix_last(ch, last_poly):
    """last_poly uint32[n, 4] -> the channel after the coefficients, two per mix."""
    c = np.asarray(last_poly, dtype=np.uint32).reshape(-1, 4)
    for i in range(0, len(c), 2):
        if i + 1 < len(c):
            ch.mix(list(c[i]) + list(c[i + 1]))
        else:
            ch.mix_one(list(c[i]))


def begin(ch, samples):
    """samples uint32[142, 4]: mix them two per mix, draw `after`."""
    s = np.asarray(samples, dtype=np.uint32).reshape(-1, 4)
    for i in range(0, len(s), 2):
        ch.mix(list(s[i]) + list(s[i + 1]))
    return ch.draw()[0]


def n_inner_of(M, log_last, b):
    return M - 1 - log_last - b


def commit(cols, log_last, b, ch, ob):
    """cols {LDE log size: QM31 column (4, 2^size)}, ch a commit_ref.Channel (updated) -> dict of roots [1 + n_inner][8],
    alphas, layers (list of (4, 2^l)), last_poly uint32[2^log_last, 4], low_degree."""
    M = max(cols)
    L = log_last + b
    assert min(cols) - b > log_last
    roots, alphas, layers = [], [], []
    roots.append(layer_root(cols, ob))
    ch.mix(roots[-1])
    alphas.append(ch.draw()[0])
    ev = fold_circle(cols[M], M, alphas[0])
    for i in range(n_inner_of(M, log_last, b)):
        l = M - 1 - i
        layers.append(ev)
        roots.append(layer_root({l: ev}, ob))
        ch.mix(roots[-1])
        alphas.append(ch.draw()[0])
        a = alphas[-1]
        ev = fold_line(ev, l, a)
        if l in cols:
            ev = R.q_add(R.q_mul(R.q_mul(qs(a), qs(a)), ev), fold_circle(cols[l], l, a))
    assert ev.shape[1] == 1 << L
    co = line_interpolate(ev, L)
    last = np.ascontiguousarray(line_order(co[:, :1 << log_last], log_last).T, dtype=np.uint32)
    mix_last(ch, last)
    return {"roots": np.array(roots, dtype=np.uint32), "alphas": np.array(alphas, dtype=np.uint32), "layers": layers, "last_poly": last,
            "low_degree": int(not co[:, 1 << log_last:].any())}


# The cases of tests/test_fri_gpu.py::test_commit_bit_for_bit
CCASES = {  # name: (sizes, log_last, b, n, mask, low degree input)
    "three_columns": ([7, 6, 5], 2, 1, 2, None, False),
    "joins_at_the_last_fold": ([6, 4], 1, 2, 3, [1, 0, 1], False),
    "log_last_0": ([5, 3], 0, 1, 1, None, False),
    "no_inner_layer": ([4], 2, 1, 1, None, False),
    "levels_past_one_workgroup": ([11, 9], 1, 1, 1, None, False),
    "low_degree": ([8, 7, 5], 2, 2, 2, None, True),
    "past_one_workgroup_of_proofs": ([5, 3], 0, 1, 70, masked_past_64(), False),  # k_fr_draw, k_fr_mix_last
}


# ---- what tests/test_fri_gpu.py and tests/test_workspace_fill_gpu.py share of rsv_fri_quotients_dev: the restatement of one
# proof's d_quot, the cases, and their random inputs
def ref_quotients(groups, gpoints, b, points, samples, after):
    """One proof.  groups [(log, int64[n_cols, 2^log])], gpoints per group per point (lo, hi) or None, points uint32[k, 8],
    samples uint32[k, total, 4] -> uint32 words of d_quot: the columns in descending size, each [4][2^(log + b)]."""
    out, col0 = [], np.cumsum([0] + [g[1].shape[0] for g in groups])
    for size in sorted({log for log, _ in groups}, reverse=True):
        mine = [i for i, (log, _) in enumerate(groups) if log == size]
        first = np.cumsum([0] + [groups[i][1].shape[0] for i in mine])
        batches = []
        for k in range(points.shape[0]):
            terms = []
            for j, i in enumerate(mine):
                r = gpoints[i][k] if k < len(gpoints[i]) else None
                if r is not None:
                    terms += [(first[j] + c, samples[k, col0[i] + c]) for c in range(r[0], r[1])]
            batches.append(((points[k, :4], points[k, 4:]), terms))
        rows = np.concatenate([C.lde(groups[i][1], size, b) for i in mine])
        x, y = domain_xy(size + b)
        out.append(row_quotient(rows, quotient_consts(batches, after), x, y).reshape(-1))
    return np.concatenate(out).astype(np.uint32)


ALL = lambda nc: (0, nc)  # noqa: E731
QCASES = {  # name: (b, n, mask, [(log, n_cols, shared, [per point (lo, hi) or None])])
    "three_sizes_A_above_B": (1, 2, None, [(6, 8, False, [ALL(8)]), (5, 3, False, [ALL(3)]), (4, 5, False, [ALL(5)]),
                                           (5, 4, False, [ALL(4), (2, 4)]), (4, 4, False, [ALL(4), None, (1, 3)])]),
    "three_sizes_A_below_B": (2, 3, [1, 0, 1], [(6, 8, False, [ALL(8)]), (3, 3, False, [ALL(3)]), (4, 5, False, [ALL(5)]),
                                                (3, 4, False, [ALL(4), (2, 4)]), (4, 4, False, [ALL(4), None, (1, 3)])]),
    "equal_sizes_merge": (1, 2, None, [(6, 8, False, [ALL(8)]), (4, 3, False, [ALL(3)]), (4, 5, False, [ALL(5)]),
                                       (4, 4, False, [ALL(4), (2, 4)]), (4, 4, False, [ALL(4), (0, 4)])]),
    "shared_group": (1, 3, None, [(5, 6, True, [ALL(6)]), (5, 2, False, [ALL(2), (1, 2)])]),
    "past_the_lds_fft": (1, 1, None, [(11, 2, False, [ALL(2), (0, 1)])]),
    "past_one_workgroup_of_proofs": (1, 70, None, [(4, 3, False, [ALL(3), (1, 3)]), (3, 2, False, [ALL(2)])]),  # k_fr_consts
}


def qinputs(rng, spec, n, value=None):
    draw = (lambda shape: rng.integers(0, P, shape)) if value is None else (lambda shape: np.full(shape, value, np.int64))
    groups = [(log, draw((1 if sh else n, nc, 1 << log))) for log, nc, sh, _ in spec]
    k = max(len(g[3]) for g in spec)
    total = sum(g[1] for g in spec)
    return groups, [g[3] for g in spec], draw((n, k, 8)).astype(np.uint32), draw((n, k, total, 4)).astype(np.uint32), draw((n, 4)).astype(np.uint32)
