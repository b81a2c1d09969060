"""Test helper (numpy, no device): commitment of a tree of the next proof, restated from stwo's conventions.

- Columns are M31 evaluations on CanonicCoset(log).circle_domain(), stored in bit-reversed order (as k_trace and
  k_interaction store them).  `interpolate` gives the CirclePoly coefficients: coefficient i multiplies
  y^{i_0} x^{i_1} pi(x)^{i_2} pi^2(x)^{i_3} ..., i_k = bit k of i, pi(x) = 2x^2 - 1 (the fold order of
  CirclePoly::eval_at_point).  `evaluate` is the low-degree extension: the same coefficients, zero-padded, on
  CanonicCoset(log + b).circle_domain(), bit-reversed.
- In bit-reversed storage, butterfly layer m pairs positions p and p + 2^m (bit m of p clear); its twiddle is, for layer
  0, the y and, for layer m >= 1, the x of 2^(m-1) * half_coset.at(bitrev(p >> (m + 1) << m)), the half coset being
  Coset::half_odds(N - 1) of the domain of size 2^N.
- `merkle_root`: stwo's mixed-size Merkle rule (oracle/rsv_oracle.c verify_trace_tree), hashed through the oracle's
  hash_node over whole layers.
- `transcript_prefix`: the next transcript's prefix (oracle/rsv_oracle.c run_transcript) through the oracle's
  half_permute: mix root 0, lp, lq, root 1, draw (z, alpha), mix the two claimed sums, root 2, draw random_coeff."""
import functools

import numpy as np

P = 0x7FFFFFFF
GEN = (2, 1268011823)


def _gen_table():
    t, (x, y) = [], GEN
    for _ in range(31):
        t.append((x, y))
        x, y = (x * x - y * y) % P, (2 * x * y) % P
    return t


_GT = _gen_table()


def gen_mul(k):
    """k * GEN for an int64 array k (mod 2^31) -> (x, y) int64 arrays."""
    k = np.asarray(k, dtype=np.int64) & ((1 << 31) - 1)
    x, y = np.ones_like(k), np.zeros_like(k)
    for i, (gx, gy) in enumerate(_GT):
        bit = ((k >> i) & 1).astype(bool)
        nx, ny = (x * gx - y * gy) % P, (x * gy + y * gx) % P
        x, y = np.where(bit, nx, x), np.where(bit, ny, y)
    return x, y


def bit_reverse(v, bits):
    v = np.asarray(v, dtype=np.int64)
    r = np.zeros_like(v)
    for b in range(bits):
        r |= ((v >> b) & 1) << (bits - 1 - b)
    return r


@functools.lru_cache(maxsize=None)
def twiddles(N, m):
    """Layer m twiddles of the domain of size 2^N: int64[2^(N-1-m)]."""
    k = np.arange(1 << (N - 1 - m), dtype=np.int64)
    idx = (1 << (30 - N)) + bit_reverse(k << m if m else k, N - 1) * (1 << (32 - N))
    if m == 0:
        return gen_mul(idx)[1]
    return gen_mul(idx << (m - 1))[0]


def _m_inv(a):
    r, b, e = np.ones_like(a), a % P, P - 2
    while e:
        if e & 1:
            r = r * b % P
        b = b * b % P
        e >>= 1
    return r


@functools.lru_cache(maxsize=None)
def _inv_twiddles(N, m):
    return _m_inv(twiddles(N, m))


def interpolate(cols, log):
    """int64[..., 2^log] evaluations (bit-reversed) -> coefficients."""
    v = np.array(cols, dtype=np.int64) % P
    shape = v.shape
    for m in range(log):
        it = _inv_twiddles(log, m)
        v = v.reshape(-1, 1 << (log - 1 - m), 2, 1 << m)
        a, b = v[:, :, 0, :], v[:, :, 1, :]
        a, b = (a + b) % P, (a - b) % P * it[None, :, None] % P
        v = np.stack([a, b], axis=2)
    return v.reshape(shape) * pow(2, (31 - log) % 31, P) % P


def evaluate(coeffs, log, N):
    """int64[..., 2^log] coefficients -> int64[..., 2^N] evaluations on CanonicCoset(N).circle_domain(), bit-reversed."""
    c = np.asarray(coeffs, dtype=np.int64) % P
    lead = c.shape[:-1]
    v = np.zeros(lead + (1 << N,), np.int64)
    v[..., :1 << log] = c
    for m in reversed(range(N)):
        t = twiddles(N, m)
        v = v.reshape(-1, 1 << (N - 1 - m), 2, 1 << m)
        a, b = v[:, :, 0, :], v[:, :, 1, :] * t[None, :, None] % P
        v = np.stack([(a + b) % P, (a - b) % P], axis=2)
    return v.reshape(lead + (1 << N,))


def lde(cols, log, b):
    return evaluate(interpolate(cols, log), log, log + b)


def eval_at_point(coeffs, log, point):
    """CirclePoly::eval_at_point of coefficients int64[2^log] at a QM31 point ((x0..x3), (y0..y3)) -> QM31 tuple."""
    from tests import interaction_ref as R
    x, y = R.q(point[0]), R.q(point[1])
    vals = R.m31(np.asarray(coeffs, dtype=np.int64) % P)  # QM31 array (4, 2^log)
    folds = [y, x]
    for _ in range(2, log):
        folds.append(R.q_sub(R.q_mul_m(R.q_mul(folds[-1], folds[-1]), 2), R.q((1, 0, 0, 0))))
    for k in range(log):
        vals = vals.reshape(4, -1, 2)
        vals = R.q_add(vals[:, :, 0], R.q_mul(vals[:, :, 1], folds[k]))
    return tuple(int(t) for t in vals[:, 0])


def merkle_root(layers, ob):
    """layers: {log size: uint32/int64 [n_cols, 2^log]} (columns in commitment order) -> uint32[8]."""
    top = max(layers)
    cur = None
    for l in range(top, -1, -1):
        cols = layers.get(l)
        c = np.zeros((1 << l, 0), np.uint32) if cols is None else np.ascontiguousarray(np.asarray(cols, dtype=np.int64).T % P, dtype=np.uint32)
        if cur is None:
            cur = ob.hash_node(None, c)
        else:
            pairs = cur.reshape(-1, 2, 8)
            cur = ob.hash_node((np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])), c)
    return cur[0]


def tree_layers(groups, b):
    """[(log, int64[n_cols, 2^log] columns)] in group order -> {log + b: LDE columns} (groups of equal size concatenated)."""
    out = {}
    for log, cols in groups:
        e = lde(cols, log, b)
        out[log + b] = e if log + b not in out else np.concatenate([out[log + b], e])
    return out


def commit(groups, b, ob):
    return merkle_root(tree_layers(groups, b), ob)


class Channel:
    """ChannelVar through the oracle's half_permute: digest[8], n_sent."""

    def __init__(self, ob, digest=None, n_sent=0):
        self.ob, self.digest, self.n_sent = ob, np.zeros(8, np.uint32) if digest is None else np.asarray(digest, np.uint32), n_sent

    def mix(self, words8):
        _, cap = self.ob.half_permute(np.asarray(words8, np.uint32).reshape(1, 8), self.digest.reshape(1, 8))
        self.digest, self.n_sent = cap[0], 0

    def mix_one(self, q4):
        self.mix(list(q4) + [0, 0, 0, 0])

    def draw(self):
        l = np.zeros(8, np.uint32)
        l[0] = self.n_sent
        self.n_sent += 1
        rate, _ = self.ob.half_permute(l.reshape(1, 8), self.digest.reshape(1, 8))
        return tuple(int(x) for x in rate[0, :4]), tuple(int(x) for x in rate[0, 4:])


def transcript_prefix(roots, lp, lq, sums, ob):
    """roots: three uint32[8]; sums: (plonk QM31, poseidon QM31) -> (z, alpha, random_coeff, channel)."""
    ch = Channel(ob)
    ch.mix(roots[0])
    ch.mix_one((lp, 0, 0, 0))
    ch.mix_one((lq, 0, 0, 0))
    ch.mix(roots[1])
    z, alpha = ch.draw()
    ch.mix(list(sums[0]) + list(sums[1]))
    ch.mix(roots[2])
    rc, _ = ch.draw()
    return z, alpha, rc, ch


def query_positions(proof, ob):
    """(the transcript's query positions at the largest log size M, M) of a proof."""
    tr = ob.transcript_raw(proof)
    n_layers, nq, M = int(tr[1]), int(tr[2]), int(tr[3])
    raw = tr[40 + 4 * n_layers:40 + 4 * n_layers + nq].astype(np.int64)
    return raw & ((1 << M) - 1), M


def decommitted(layers, q_at_max):
    """The values of one query at a tree's layers as SinglePathMerkleProof::columns orders them (largest layer first)."""
    top = max(layers)
    out = []
    for l in range(top, -1, -1):
        if l in layers:
            out.extend(int(v) for v in np.asarray(layers[l])[:, q_at_max >> (top - l)])
    return out
