"""Test helper (numpy, no device): the sampled values of committed columns, restated over tests/commit_ref.py.

`sample_tree` interpolates the columns (commit_ref.interpolate) and evaluates every column at every point; the value is
CirclePoly::eval_at_point (commit_ref.eval_at_point), computed as a dot product with the weight vector W_i = prod_k
f_k^{i_k}, f_0 = y, f_1 = x, f_{k+1} = 2 f_k^2 - 1, made once per (log, point).  tests/test_sample_host.py pins the
dot-product form to eval_at_point and to the oracle's PointEvaluator, and `witness_samples` (the proof's own order) to the
reference's fixtures; tests/test_sample_gpu.py compares the device against this helper."""
import numpy as np

from tests import commit_ref as C
from tests import interaction_ref as R

P = C.P


def weights(log, point):
    """int64[4, 2^log]: W_i of the QM31 point ((x0..x3), (y0..y3)); any integer words, taken mod P."""
    f = R.q(point[1])
    w = R.q((1, 0, 0, 0))
    for k in range(log):
        w = np.concatenate([w, R.q_mul(w, f)], axis=1)
        f = R.q(point[0]) if k == 0 else R.q_sub(R.q_mul_m(R.q_mul(f, f), 2), R.q((1, 0, 0, 0)))
    return w


def dot(coeffs, w):
    """int64[..., 2^log] coefficients x weights int64[4, 2^log] -> int64[..., 4]."""
    c = np.asarray(coeffs, dtype=np.int64) % P
    return np.stack([(c * w[j] % P).sum(axis=-1) % P for j in range(4)], axis=-1)


def sample_coeffs(groups, points):
    """[(log, int64[n_cols, 2^log] coefficients)], [point] -> uint32[n_points, sum n_cols, 4]."""
    out = []
    for pt in points:
        out.append(np.concatenate([dot(co, weights(log, pt)) for log, co in groups]))
    return np.array(out, dtype=np.uint32)


def sample_tree(groups, points):
    """[(log, int64[n_cols, 2^log] evaluations, bit-reversed)], [point] -> uint32[n_points, sum n_cols, 4]."""
    return sample_coeffs([(log, C.interpolate(cols, log)) for log, cols in groups], points)


def witness_samples(trees, oods):
    """trees: the three trees' groups [(log, evaluations)] in commitment order (tree 2: the two components' 8 interaction
    columns) -> uint32[134, 4], sampled_values[0..2] in the proof's own order: tree-major, column-major, sample-minor; tree
    2's columns 4..7 at the previous-row point of their component's size, then at the OODS point."""
    out = []
    for t, groups in enumerate(trees):
        for log, cols in groups:
            co = C.interpolate(cols, log)
            at = dot(co, weights(log, oods))
            if t < 2:
                out.extend(at)
                continue
            prev = dot(co, weights(log, R.prev_row_point(oods, log)))
            for k in range(len(co)):
                out.extend([at[k]] if k < 4 else [prev[k], at[k]])
    return np.array(out, dtype=np.uint32)


def flatten_samples(sampled_values):
    """parse_proof's sampled_values[0..2] -> uint32[134, 4] in the proof's order."""
    return np.array([v for t in range(3) for col in sampled_values[t] for v in col], dtype=np.uint32)


# The trees of tests/test_sample_gpu.py::test_sample_tree_path_switches, as chain_harness.CASES: (groups as (log, cols, shared), b, n, mask)
SWITCHES = [  # both sides of 2^8 (idle lanes), 2^10 (the unrolled loop) and 2^13 (chunks per column), up to 2^16
    ([(7, 2, False), (8, 3, False)], 1, 2, None),
    ([(9, 2, False), (10, 2, False), (11, 1, False)], 1, 2, [1, 0]),
    ([(12, 2, False), (13, 2, False)], 1, 2, None),
    ([(14, 2, True), (13, 1, False)], 1, 3, [1, 1, 0]),
    ([(15, 1, False)], 1, 2, None),
    ([(16, 1, False)], 1, 1, None),
]
