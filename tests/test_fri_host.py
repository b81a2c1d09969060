"""tests/fri_ref.py pinned to the reference on one fixture, without a device and without the full domain: the row quotient of
the proof's own queried values against the oracle's per-query answers, the folds of the proof's own (value, sibling) pairs
against the oracle's folded values, the line interpolation against the oracle's line_eval, the restated channel against the
oracle's transcript, and the host refusals of rsv_fri_sizes."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import fri_ref as F
from tests import interaction_ref as R
from tests import oracle_binding as ob
from tests.chain_harness import pow_words
from tests.conftest import read_proof

FIXTURE = "level1-5.bin"
P = C.P


@pytest.fixture(scope="module")
def proof():
    pr = read_proof(FIXTURE)
    lay = ob.proof_layout(pr)
    tr = ob.transcript_raw(pr)
    lp, lq, b, log_last = lay["lp"], lay["lq"], lay["blowup"], lay["log_last"]
    M = int(tr[3])
    assert M == max(lp + 1, lq + 2) + b
    w = np.frombuffer(pr, dtype=np.uint32)
    at = next(pos for pos, _, what in lay["prefixes"] if what == "last_layer_poly")
    last = w[at + 2:at + 2 + 4 * (1 << log_last)].reshape(-1, 4).copy()
    qM, M2 = C.query_positions(pr, ob)
    assert M2 == M
    return {"proof": pr, "lp": lp, "lq": lq, "b": b, "log_last": log_last, "M": M, "n_inner": lay["n_inner"], "tr": tr, "last": last,
            "roots": lay["fri_commitments"], "qM": qM, "samples": ob.sampled_values(pr), "dump": ob.query_dump(pr),
            "alphas": [tuple(int(v) for v in tr[40 + 4 * i:44 + 4 * i]) for i in range(lay["n_inner"] + 1)]}


def _chain_batches(d, size):
    """The batches of the size's quotient column in the proof's own sample order (verify_one's group_add_cols)."""
    s, lp, lq, b, M = d["samples"], d["lp"], d["lq"], d["b"], d["M"]
    oods = (tuple(int(v) for v in d["tr"][20:24]), tuple(int(v) for v in d["tr"][24:28]))
    if size == M:
        return [(oods, [(c, s[134 + c]) for c in range(8)])]
    zero, prev, col = [], [], 0
    for t, (np_cols, nq_cols, base) in enumerate(((10, 40, 0), (12, 48, 50), (8, 8, 110))):
        for comp, (n_cols, off, log) in enumerate(((np_cols, base, lp), (nq_cols, base + (np_cols if t < 2 else 12), lq))):
            if log + b != size:
                continue
            for c in range(n_cols):
                if t < 2 or c < 4:
                    zero.append((col, s[off + c]))
                else:
                    prev.append((col, s[off + 4 + 2 * (c - 4)], log))
                    zero.append((col, s[off + 5 + 2 * (c - 4)]))
                col += 1
    out = [(oods, zero)]
    if prev:
        out.append((R.prev_row_point(oods, prev[0][2]), [(c, v) for c, v, _ in prev]))
    return out


def _sizes(d):
    A, B = d["lp"] + d["b"], d["lq"] + d["b"]
    return [d["M"]] + ([A] if A == B else [max(A, B), min(A, B)])


def test_row_quotient_of_the_queried_values(proof):
    """Per size and query: the proof's queried columns (trace_cols), its samples and `after` give the oracle's answers."""
    d = proof
    cols = ob.trace_cols(d["proof"])
    after = tuple(int(v) for v in d["tr"][28:32])
    A, B, M = d["lp"] + d["b"], d["lq"] + d["b"], d["M"]
    nq = len(d["qM"])
    for gi, size in enumerate(_sizes(d)):
        if size == M:
            rows = cols[3, :, :8].T
        else:
            parts = []
            for t, (pc, qc) in enumerate(((10, 40), (12, 48), (8, 8))):
                # a tree's queried columns: the larger size's first, then the smaller's
                first_is_plonk = A >= B
                lo, hi = (pc, qc) if first_is_plonk else (qc, pc)
                big, small = cols[t, :, :lo], cols[t, :, lo:lo + hi]
                plonk, poseidon = (big, small) if first_is_plonk else (small, big)
                if A == B:
                    plonk, poseidon = cols[t, :, :pc], cols[t, :, pc:pc + qc]
                if size == A:
                    parts.append(plonk)
                if size == B:
                    parts.append(poseidon)
            rows = np.concatenate(parts, axis=1).T
        pos = d["qM"] >> (M - size)
        x, y = F.domain_xy(size, pos)
        got = F.row_quotient(rows, F.quotient_consts(_chain_batches(d, size), after), x, y)
        assert np.array_equal(got.T, d["dump"][:, 4 * gi:4 * gi + 4].astype(np.int64)), size
    assert nq == d["dump"].shape[0]


def test_folds_of_the_proofs_own_pairs(proof):
    """The circle-to-line fold of every first-layer pair equals fri_folded; the running evaluation through the inner layers
    (fold of the pair, then the joining column) equals the values the oracle sees entering each layer and the last check."""
    d = proof
    M, ni, sizes = d["M"], d["n_inner"], _sizes(d)
    _, pairs = ob.fri_paths(d["proof"], len(d["qM"]), M, 1 + ni)
    folded = ob.fri_folded(d["proof"])
    first = {}
    for gi, size in enumerate(sizes):
        pos = d["qM"] >> (M - size)
        me, sib = pairs[0, :, gi, :4].astype(np.int64).T, pairs[0, :, gi, 4:].astype(np.int64).T
        odd = (pos & 1).astype(bool)
        f0, f1 = np.where(odd, sib, me), np.where(odd, me, sib)
        y = F.domain_xy(size, pos & ~1)[1]
        first[size] = F.fold_pairs(f0, f1, d["alphas"][M - size], y)
        assert np.array_equal(first[size].T, folded[gi].astype(np.int64)), size
    ev = first[M]
    for i in range(ni):
        l = M - 1 - i
        assert np.array_equal(ev.T, d["dump"][:, 24 + 4 * i:28 + 4 * i].astype(np.int64)), i
        pos = d["qM"] >> (M - l)
        me, sib = pairs[1 + i, :, 0, :4].astype(np.int64).T, pairs[1 + i, :, 0, 4:].astype(np.int64).T
        assert np.array_equal(me, ev)
        odd = (pos & 1).astype(bool)
        a = d["alphas"][i + 1]
        ev = F.fold_pairs(np.where(odd, sib, me), np.where(odd, me, sib), a, F.line_x(l, pos >> 1))
        if l in first and i + 1 < ni:
            ev = R.q_add(R.q_mul(R.q_mul(F.qs(a), F.qs(a)), ev), first[l])
    assert np.array_equal(ev.T, d["dump"][:, 24 + 4 * ni:28 + 4 * ni].astype(np.int64))


def test_line_interpolation_round_trip(proof):
    """line_eval of the proof's last_poly on the last domain, interpolated by the restatement, gives last_poly back, and
    zeros past it."""
    d = proof
    L = d["log_last"] + d["b"]
    ev = ob.line_eval(d["last"], _last_domain_x(L))
    co = F.line_interpolate(ev.astype(np.int64).T, L)
    assert not co[:, 1 << d["log_last"]:].any()
    assert np.array_equal(F.line_order(co[:, :1 << d["log_last"]], d["log_last"]).T, d["last"].astype(np.int64))


def _last_domain_x(L):
    """x of half_odds(L).at(bit_reverse(i, L)) for every storage position i of a line layer of log size L."""
    return np.ascontiguousarray(F.domain_xy(L + 1, 2 * np.arange(1 << L, dtype=np.int64))[0], dtype=np.uint32)


def test_channel_run(proof):
    """From the channel behind the OODS draw (rebuilt from the proof's roots): the samples give `after` (word 28), the FRI
    roots the alphas (words 40..), and the nonce mixed behind last_poly gives the proof-of-work digest (words 32..39)."""
    d = proof
    w = np.frombuffer(d["proof"], dtype=np.uint32)
    roots = [w[17 + 8 * t:25 + 8 * t] for t in range(4)]
    sums = (tuple(int(v) for v in w[2:6]), tuple(int(v) for v in w[6:10]))
    z, alpha, rc, ch = C.transcript_prefix(roots[:3], d["lp"], d["lq"], sums, ob)
    assert list(z) + list(alpha) + list(rc) == [int(v) for v in d["tr"][4:16]]
    ch.mix(roots[3])
    assert list(ch.draw()[0]) == [int(v) for v in d["tr"][16:20]]
    assert list(F.begin(ch, d["samples"])) == [int(v) for v in d["tr"][28:32]]
    for i, root in enumerate(d["roots"]):
        ch.mix(root)
        assert ch.draw()[0] == d["alphas"][i], i
    F.mix_last(ch, d["last"])
    ch.mix_one(pow_words(d["proof"]))
    assert [int(v) for v in ch.digest] == [int(v) for v in d["tr"][32:40]]


def test_fri_sizes_and_refusals(rsv):
    """rsv_fri_sizes: the sizes, the layer count and the buffer words; RSV_E_SIZE for what the device calls refuse."""
    got = rsv.fri_sizes(10, 9, 1, 0)
    assert got == {"sizes": [12, 11, 10], "n_inner": 10, "quot_words": 4 * (4096 + 2048 + 1024), "layer_words": 4 * (4096 - 4), "last_words": 4}
    assert rsv.fri_sizes(7, 6, 2, 3) == {"sizes": [10, 9, 8], "n_inner": 4, "quot_words": 4 * (1024 + 512 + 256),
                                         "layer_words": 4 * (512 + 256 + 128 + 64), "last_words": 32}
    assert rsv.fri_sizes(6, 5, 1, 4)["sizes"] == [8, 7, 6] and rsv.fri_sizes(5, 5, 1, 4)["sizes"] == [8, 6]
    assert rsv.fri_sizes(5, 6, 1, 4)["sizes"] == [9, 7, 6]
    for bad in ((10, 9, 1, 9), (9, 10, 1, 9), (10, 9, 1, 17), (10, 9, 0, 0), (10, 9, 17, 0), (1, 9, 1, 0), (10, 1, 1, 0), (28, 9, 2, 0),
                (29, 9, 1, 0)):
        with pytest.raises(rsv.RsvError) as e:
            rsv.fri_sizes(*bad)
        assert e.value.code == -2, bad
