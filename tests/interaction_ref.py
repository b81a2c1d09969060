"""Test helper (numpy, no device): the recursion circuit's interaction (logup) columns, restated from the AIR the verifier
evaluates (oracle/recursion_circuit/verifier.py: EvalAtRow.add_to_relation / finalize_logup, evaluate_plonk,
evaluate_poseidon).  tests/test_interaction_host.py pins it to the reference's fixtures; tests/test_interaction_gpu.py
compares the device's columns against it.

Per component, two secure columns (4 M31 coordinate columns each, combine_ef order): column 0 = the first batch's
fraction sum at the row; column 1 = S[k] = sum_{j <= k} (f0[j] + f1[j] - shift) in the domain's coset order, shift =
total / 2^log_size, total = the claimed sum.  Rows are stored like the trace: position i = the i-th value of the
bit-reversed circle-domain evaluation."""
import numpy as np

P = 0x7FFFFFFF


# ---------------------------------------------------------------- QM31 on int64 arrays of shape (4, n)
def q(c, n=None):
    """A constant QM31 (4-tuple) broadcast to (4, 1)."""
    return np.array([int(x) % P for x in c], dtype=np.int64).reshape(4, 1)


def m31(col):
    """An M31 column as a QM31 array (x, 0, 0, 0)."""
    col = np.asarray(col, dtype=np.int64) % P
    z = np.zeros_like(col)
    return np.stack([col, z, z, z])


def q_add(x, y):
    return (x + y) % P


def q_sub(x, y):
    return (x - y) % P


def q_mul_m(x, k):
    return x * (np.asarray(k, dtype=np.int64) % P) % P


def _c_mul(a0, a1, b0, b1):
    return (a0 * b0 % P - a1 * b1 % P) % P, (a0 * b1 % P + a1 * b0 % P) % P


def q_mul(x, y):
    x, y = np.broadcast_arrays(x, y)
    ac = _c_mul(x[0], x[1], y[0], y[1])
    bd = _c_mul(x[2], x[3], y[2], y[3])
    ad = _c_mul(x[0], x[1], y[2], y[3])
    bc = _c_mul(x[2], x[3], y[0], y[1])
    # u^2 = 2 + i: bd * (2 + i) = (2 bd0 - bd1) + (2 bd1 + bd0) i
    return np.stack([(ac[0] + 2 * bd[0] - bd[1]) % P, (ac[1] + 2 * bd[1] + bd[0]) % P, (ad[0] + bc[0]) % P, (ad[1] + bc[1]) % P])


def _m_pow(x, e):
    r = np.ones_like(x)
    b = x % P
    while e:
        if e & 1:
            r = r * b % P
        b = b * b % P
        e >>= 1
    return r


def q_inv(x):
    """1 / x (0 for x = 0)."""
    # (a + b u)^-1 = (a - b u) / (a^2 - (2 + i) b^2)
    a2 = _c_mul(x[0], x[1], x[0], x[1])
    b2 = _c_mul(x[2], x[3], x[2], x[3])
    rb2 = ((2 * b2[0] - b2[1]) % P, (2 * b2[1] + b2[0]) % P)
    d0, d1 = (a2[0] - rb2[0]) % P, (a2[1] - rb2[1]) % P
    n = _m_pow((d0 * d0 + d1 * d1) % P, P - 2)
    i0, i1 = d0 * n % P, (-d1) % P * n % P
    r0 = _c_mul(x[0], x[1], i0, i1)
    r1 = _c_mul((-x[2]) % P, (-x[3]) % P, i0, i1)
    return np.stack([r0[0], r0[1], r1[0], r1[1]])


def is_zero(x):
    return (x == 0).all(axis=0)


# ---------------------------------------------------------------- relations
def _denom(z, alpha, alpha2, values):
    """sum_i alpha^i values[i] - z (values: QM31 arrays)."""
    d = values[0]
    if len(values) > 1:
        d = q_add(d, q_mul(alpha, values[1]))
    if len(values) > 2:
        d = q_add(d, q_mul(alpha2, values[2]))
    return q_sub(d, z)


def _batch(entries):
    """[(multiplicity M31 column, denominator)] -> (p, q) as finalize_logup combines a batch."""
    p, qq = m31(entries[0][0]), entries[0][1]
    for m, d in entries[1:]:
        p = q_add(q_mul(p, d), q_mul_m(qq, m))
        qq = q_mul(qq, d)
    return p, qq


def plonk_batches(pre, trace, z, alpha):
    """pre: [10, N] (trace.PREPROCESSED order), trace: [12, N] -> ((p0, q0), (p1, q1))."""
    z, alpha = q(z), q(alpha)
    alpha2 = q_mul(alpha, alpha)
    pre = np.asarray(pre, dtype=np.int64) % P
    trace = np.asarray(trace, dtype=np.int64) % P
    a_val, b_val, c_val = trace[0:4], trace[4:8], trace[8:12]
    ea = (pre[4], _denom(z, alpha, alpha2, [a_val, m31(pre[0])]))
    eb = (pre[5], _denom(z, alpha, alpha2, [b_val, m31(pre[1])]))
    ec = (pre[6], _denom(z, alpha, alpha2, [c_val, m31(pre[2])]))
    ep = ((-pre[8]) % P, _denom(z, alpha, alpha2, [m31(pre[7]), a_val, b_val]))
    return _batch([ea, eb]), _batch([ec, ep])


def poseidon_batches(pre, trace, z, alpha):
    """pre: [40, N], trace: [48, N] (in, intermediate, out) -> ((p0, q0), (p1, q1))."""
    z, alpha = q(z), q(alpha)
    alpha2 = q_mul(alpha, alpha)
    pre = np.asarray(pre, dtype=np.int64) % P
    tr = np.asarray(trace, dtype=np.int64) % P
    first, last, rid = pre[0], pre[1], pre[3]
    ext1, ext2, nz1, nz2 = pre[36], pre[37], pre[38], pre[39]
    not_first, not_last = (1 - first) % P, (1 - last) % P
    m = lambda a, b: a * b % P
    ins, outs = tr[0:16], tr[32:48]
    e = []
    for h, (sel_nz, ext) in enumerate(((nz1, ext1), (nz2, ext2))):
        ident = (m(first, ext) + m(not_first, (2 * rid + h) % P)) % P
        e.append(((m(sel_nz, first) - not_first) % P, _denom(z, alpha, alpha2, [m31(ident), ins[8 * h:8 * h + 4], ins[8 * h + 4:8 * h + 8]])))
    for h, (sel_nz, ext) in enumerate(((nz1, ext1), (nz2, ext2))):
        ident = (m(last, ext) + m(not_last, (2 * rid + 2 + h) % P)) % P
        e.append(((m(sel_nz, last) + not_last) % P, _denom(z, alpha, alpha2, [m31(ident), outs[8 * h:8 * h + 4], outs[8 * h + 4:8 * h + 8]])))
    e.append((m(first, not_last), _denom(z, alpha, alpha2, [m31(tr[16]), m31(pre[4])])))
    return _batch(e[0:3]), _batch(e[3:5])


# ---------------------------------------------------------------- columns
def coset_positions(log_n):
    """pos[k] = storage position of coset index k: circle-domain index k / 2 (even k) or (2^(n+1) - k) / 2 (odd k),
    bit-reversed over n bits."""
    N = 1 << log_n
    k = np.arange(N, dtype=np.int64)
    d = np.where(k % 2 == 0, k // 2, (2 * N - k) // 2)
    rev = np.zeros_like(d)
    for b in range(log_n):
        rev |= ((d >> b) & 1) << (log_n - 1 - b)
    return rev


def columns(batches, log_n):
    """-> (int64[8, N] columns, total QM31 tuple, ok).  ok is False if a denominator is zero; the columns and total are
    then zero (the library's convention)."""
    (p0, q0), (p1, q1) = batches
    N = 1 << log_n
    if is_zero(q0).any() or is_zero(q1).any():
        return np.zeros((8, N), np.int64), (0, 0, 0, 0), False
    f0 = q_mul(p0, q_inv(q0))
    f1 = q_mul(p1, q_inv(q1))
    g = q_add(f0, f1)
    total = g.sum(axis=1) % P
    shift = total * pow(N, P - 2, P) % P
    pos = coset_positions(log_n)
    gk = (g[:, pos] - shift[:, None]) % P
    S = np.cumsum(gk, axis=1) % P  # N * P < 2^63
    col1 = np.zeros_like(S)
    col1[:, pos] = S
    return np.concatenate([f0, col1]).astype(np.int64), tuple(int(x) for x in total), True


def interaction(plonk_pre, plonk_trace, poseidon_pre, poseidon_trace, z, alpha, lp, lq):
    """-> (plonk int64[8, 2^lp], poseidon int64[8, 2^lq], sums ((plonk), (poseidon)), ok) with the library's zeroing of
    both components when any denominator of either is zero."""
    cp, sp, okp = columns(plonk_batches(plonk_pre, plonk_trace, z, alpha), lp)
    cq, sq, okq = columns(poseidon_batches(poseidon_pre, poseidon_trace, z, alpha), lq)
    if not (okp and okq):
        return np.zeros_like(cp), np.zeros_like(cq), ((0,) * 4, (0,) * 4), False
    return cp, cq, (sp, sq), True


def input_sum(inputs, z, alpha):
    """sum over the public inputs (idx, v) of 1 / (v + idx alpha - z) (fiat_shamir's balance term)."""
    acc = np.zeros((4, 1), np.int64)
    for idx, v in inputs:
        d = q_sub(q_add(q(v), q_mul_m(q(alpha), idx)), q(z))
        acc = q_add(acc, q_inv(d))
    return tuple(int(x) for x in acc[:, 0])


def prev_row_point(point, log_size):
    """point - step(log_size): the previous-row sample point (answer(): oods + step * -1)."""
    from oracle.recursion_circuit import gadgets as G
    c = G.cp_mul(G.canonic_coset(log_size).step, -1)
    x, y = point
    return (tuple((x[k] * c[0] - y[k] * c[1]) % P for k in range(4)), tuple((x[k] * c[1] + y[k] * c[0]) % P for k in range(4)))
