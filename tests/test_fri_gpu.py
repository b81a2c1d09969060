"""rsv_fri_quotients_dev / rsv_fri_commit_dev / rsv_witness_fri_dev (`-m gpu`): the commit phase of FRI of the next proof.
Against the REFERENCE for all 14 consecutive fixture pairs (the chain of fixture K gives K+1's FRI commitments, last
polynomial, `after`, alphas and a channel from which K+1's nonce gives its proof-of-work digest), a batch with a rejected
proof, bit for bit against the numpy restatement (tests/fri_ref.py, pinned to the reference by tests/test_fri_host.py) on
random columns at the smallest shapes where a path changes, a workspace budget that cuts blocks and proofs, and the
refusals.  Every comparison is exact on 32-bit words and covers every element; outputs are prefilled with 0xffffffff."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import fri_ref as F
from tests import oracle_binding as ob
from tests.chain_harness import DEV, chain, dev, full, inputs_of, mask_dev, masked_past_64, pin_id, pins, pow_words, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = C.P


def _fri(rsv, ctx, wp, batch, inputs, b, log_last):
    """The chain through witness_tree3, witness_sample and witness_fri -> (ok list, dict of numpy outputs)."""
    got = chain(rsv, ctx, wp, batch, inputs, b, upto="fri", log_last=log_last).numpy()
    return got["ok"].tolist(), got


def _want(dst):
    nxt = read_proof(dst)
    lay = ob.proof_layout(nxt)
    w = np.frombuffer(nxt, dtype=np.uint32)
    at = next(pos for pos, _, what in lay["prefixes"] if what == "last_layer_poly")
    return nxt, lay, w[at + 2:at + 2 + 4 * (1 << lay["log_last"])].reshape(-1, 4), ob.transcript_raw(nxt)


def _check_against(got, k, dst):
    nxt, lay, last, tr = _want(dst)
    ni = lay["n_inner"]
    assert got["fri_roots"].shape[1] == 1 + ni
    assert np.array_equal(got["fri_roots"][k], np.array(lay["fri_commitments"], dtype=np.uint32))
    assert np.array_equal(got["last_poly"][k], last)
    assert np.array_equal(got["after"][k], tr[28:32].astype(np.uint32))
    assert np.array_equal(got["alphas"][k].reshape(-1), tr[40:40 + 4 * (1 + ni)].astype(np.uint32))
    assert got["low_degree"][k] == 1
    ch = C.Channel(ob, got["channel"][k, :8], int(got["channel"][k, 8]))
    ch.mix_one(pow_words(nxt))
    assert np.array_equal(ch.digest, tr[32:40].astype(np.uint32))
    assert not got["channel"][k, 9:].any()


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_chain_gives_the_next_fixtures_fri_layers(rsv, pin):
    """witness_fri of fixture K: K+1's first_layer_commitment, inner_layer_commitments (and their count), last_poly,
    `after`, the alphas, low degree, and the channel its proof of work continues from."""
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    cfg = fixture_cfg(dst)
    ctx = rsv.Context(0)
    ok, got = _fri(rsv, ctx, wp, [read_proof(src)], inputs_of(src), cfg.log_blowup_factor, cfg.log_last_layer_degree_bound)
    ctx.close()
    wp.close()
    assert ok == [1]
    _check_against(got, 0, dst)
    assert not (got["quot"] == 0xFFFFFFFF).any() and not (got["layers"] == 0xFFFFFFFF).any()


def test_batch_with_a_rejected_proof(rsv):
    """Three proofs, the middle one tampered: zeros everywhere for it, the solo values for the other two."""
    pin = next(p for p in pins() if p["src"] == "level2-1.bin")
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    cfg = fixture_cfg(dst)
    proof = read_proof(src)
    ctx = rsv.Context(0)
    _, solo = _fri(rsv, ctx, wp, [proof], inputs_of(src), cfg.log_blowup_factor, cfg.log_last_layer_degree_bound)
    ok, got = _fri(rsv, ctx, wp, [proof, ob.tamper(proof, 5), proof], inputs_of(src), cfg.log_blowup_factor, cfg.log_last_layer_degree_bound)
    ctx.close()
    wp.close()
    assert ok == [1, 0, 1]
    for k in ("after", "quot", "fri_roots", "alphas", "layers", "last_poly", "low_degree", "channel"):
        assert np.array_equal(got[k][0], solo[k][0]) and np.array_equal(got[k][2], solo[k][0]), k
        assert not got[k][1].any(), k
    _check_against(solo, 0, dst)


# ---------------------------------------------------------------- rsv_fri_quotients_dev on random columns
def _run_quotients(ctx, groups, gpoints, b, n, points, samples, after, mask=None, shared=(), source=0):
    import torch
    gs = []
    for i, (log, cols) in enumerate(groups):
        gs.append({"log_size": log, "d_cols": dev(cols), "n_cols": cols.shape[-2], "proof_stride": 0 if i in shared else cols.shape[-2] << log})
    words = sum(4 << (log + b) for log in {log for log, _ in groups})
    d_quot = full((n, words))
    d_mask = mask_dev(mask)
    d_points, d_samples, d_after = dev(points), dev(samples), dev(after)
    ctx.fri_quotients(gs, gpoints, n, b, d_points, points.shape[1], d_samples, d_after, d_quot, d_mask=d_mask, source=source)
    ctx.synchronize()
    return u32(d_quot)


ALL = F.ALL
QCASES = F.QCASES


@pytest.mark.parametrize("case", list(QCASES))
def test_quotients_bit_for_bit(rsv, case):
    """Random canonical columns, points, samples and `after`: every word of d_quot equals the restatement's, the
    coefficients source gives the same words as the evaluations source, a masked proof is zero."""
    b, n, mask, spec = QCASES[case]
    rng = np.random.default_rng(1800 + list(QCASES).index(case))
    groups, gp, points, samples, after = F.qinputs(rng, spec, n)
    shared = {i for i, g in enumerate(spec) if g[2]}
    ctx = rsv.Context(0)
    got = _run_quotients(ctx, groups, gp, b, n, points, samples, after, mask, shared)
    coeffs = [(log, C.interpolate(cols, log)) for log, cols in groups]
    again = _run_quotients(ctx, coeffs, gp, b, n, points, samples, after, mask, shared, source=rsv.SAMPLE_COEFFS)
    ctx.close()
    assert np.array_equal(got, again)
    for p in range(n):
        if mask is not None and not mask[p]:
            assert not got[p].any(), p
            continue
        mine = [(log, cols[0 if i in shared else p]) for i, (log, cols) in enumerate(groups)]
        assert np.array_equal(got[p], F.ref_quotients(mine, gp, b, points[p], samples[p], after[p])), (case, p)


def test_quotients_largest_words(rsv):
    """Every column, point, sample and `after` word at P - 1."""
    b, n, _, spec = QCASES["three_sizes_A_above_B"]
    groups, gp, points, samples, after = F.qinputs(None, spec, 1, value=P - 1)
    ctx = rsv.Context(0)
    got = _run_quotients(ctx, groups, gp, b, 1, points, samples, after)
    ctx.close()
    assert np.array_equal(got[0], F.ref_quotients([(log, c[0]) for log, c in groups], gp, b, points[0], samples[0], after[0]))


def _pass_size(spec, n_points, b, n, budget):
    """The driver's pass restated (fri_api.inc: fr_ws_bytes and the two halving loops) for a one-size call -> (proofs per
    pass, blocks of 2^log rows per pass, bytes of the whole batch uncut): per group the coefficients and the extended blocks
    in flight (one set for a shared group), then 64 + 4 x terms constant words per proof; every part on a 256-byte boundary."""
    terms = sum(r[1] - r[0] for g in spec for r in g[3][:n_points] if r is not None)

    def ws(m, nb):
        parts = []
        for log, cols, sh, _ in spec:
            parts += [((1 if sh else m) * cols) << log, ((1 if sh else m) * cols * nb) << log]
        parts.append(m * (64 + 4 * terms))
        off = 0
        for words in parts:
            off = ((off + 255) & ~255) + 4 * words
        return off
    m, nb = n, 1 << b
    whole = ws(m, nb)
    while ws(m, nb) > budget and nb > 1:
        nb >>= 1
    while ws(m, nb) > budget and m > 1:
        m = (m + 1) // 2
    return m, nb, whole


def test_quotients_under_a_small_workspace_budget(rsv):
    """40 proofs of one size (2^8 rows, blowup 4): a shared group of 10 columns, groups of 12 and 8, three proofs masked.
    Uncut the call needs all four blocks of all proofs; under a 1 MB budget the driver first streams one block at a time
    (still too many bytes), then halves the proofs to 20 a pass.  _pass_size restates the driver's arithmetic and the test
    asserts the figures.  Every word of the cut run equals the uncut run, and the uncut run the restatement."""
    spec = [(8, 10, True, [ALL(10)]), (8, 12, False, [ALL(12)]), (8, 8, False, [ALL(8), (4, 8)])]
    b, n, budget = 2, 40, 1 << 20
    assert _pass_size(spec, 2, b, n, budget) == (20, 1, 4179200)
    assert _pass_size(spec, 2, b, n, 8192 << 20)[:2] == (n, 4)
    assert _pass_size(spec, 2, b, n, 1 << 21)[:2] == (n, 1)
    rng = np.random.default_rng(1820)
    groups, gp, points, samples, after = F.qinputs(rng, spec, n)
    mask = [0 if p in (0, 19, 39) else 1 for p in range(n)]
    ctx = rsv.Context(0)
    whole = _run_quotients(ctx, groups, gp, b, n, points, samples, after, mask, {0})
    ctx.set_option("ws_budget_mb", 1)
    cut = _run_quotients(ctx, groups, gp, b, n, points, samples, after, mask, {0})
    ctx.close()
    assert np.array_equal(cut, whole)
    for p in range(n):
        if not mask[p]:
            assert not whole[p].any(), p
            continue
        mine = [(log, cols[0 if i == 0 else p]) for i, (log, cols) in enumerate(groups)]
        assert np.array_equal(whole[p], F.ref_quotients(mine, gp, b, points[p], samples[p], after[p])), p


# ---------------------------------------------------------------- rsv_fri_commit_dev on random quotient columns
CCASES = F.CCASES


@pytest.mark.parametrize("case", list(CCASES))
def test_commit_bit_for_bit(rsv, case):
    """Random quotient columns (not of low degree: d_low_degree 0, last_poly still the first coefficients) or the extension
    of random low-degree polynomials (d_low_degree 1): roots, alphas, layers, last_poly, the flag and the channel equal the
    restatement's; a masked proof gets zeros and a zeroed channel."""
    import torch
    sizes, log_last, b, n, mask, low = CCASES[case]
    rng = np.random.default_rng(1840 + list(CCASES).index(case))
    if low:
        cols = [{s: C.evaluate(rng.integers(0, P, (4, 1 << (s - b))), s - b, s) for s in sizes} for _ in range(n)]
    else:
        cols = [{s: rng.integers(0, P, (4, 1 << s)) for s in sizes} for _ in range(n)]
    chan0 = np.zeros((n, 16), np.uint32)
    chan0[:, :9] = rng.integers(0, P, (n, 9))
    chan0[:, 8] %= 5
    ni = F.n_inner_of(sizes[0], log_last, b)
    lw = sum(4 << (sizes[0] - 1 - i) for i in range(ni))
    quot = np.stack([np.concatenate([c[s].reshape(-1) for s in sizes]) for c in cols])
    chan = dev(chan0)
    out = {"roots": full((n, 1 + ni, 8)), "alphas": full((n, 1 + ni, 4)), "layers": full((n, max(lw, 1))), "last": full((n, 1 << log_last, 4)),
           "low": torch.full((n,), 7, dtype=torch.uint8, device=torch.device(DEV))}
    d_mask = mask_dev(mask)
    ctx = rsv.Context(0)
    d_quot = dev(quot)
    ctx.fri_commit(d_quot, sizes, b, log_last, n, chan, out["roots"], out["alphas"], out["layers"] if ni else None, out["last"], out["low"],
                   d_mask=d_mask)
    ctx.synchronize()
    ctx.close()
    got = {k: (v.cpu().numpy() if k == "low" else u32(v)) for k, v in out.items()}
    got["chan"] = u32(chan)
    for p in range(n):
        if mask is not None and not mask[p]:
            for k in ("roots", "alphas", "last", "chan") + (("layers",) if ni else ()):
                assert not got[k][p].any(), (k, p)
            assert got["low"][p] == 0
            continue
        ch = C.Channel(ob, chan0[p, :8], int(chan0[p, 8]))
        want = F.commit(cols[p], log_last, b, ch, ob)
        assert np.array_equal(got["roots"][p], want["roots"]) and np.array_equal(got["alphas"][p], want["alphas"]), (case, p)
        if ni:
            assert np.array_equal(got["layers"][p], np.concatenate([l.reshape(-1) for l in want["layers"]]).astype(np.uint32)), (case, p)
        assert np.array_equal(got["last"][p], want["last_poly"]), (case, p)
        assert got["low"][p] == want["low_degree"] == int(low), (case, p)
        assert np.array_equal(got["chan"][p, :8], ch.digest) and got["chan"][p, 8] == ch.n_sent and not got["chan"][p, 9:].any()


def test_device_refusals(rsv):
    """NULL pointers, sizes and misalignment with a live context: the neighbours' codes, nothing written."""
    import torch
    dev = torch.device(DEV)
    ctx = rsv.Context(0)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    raw = torch.zeros(8192, dtype=torch.uint8, device=dev)
    mark = lambda *shape: torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=dev)  # noqa: E731
    # quotients: one group (3, 2 columns), blowup 1, one point
    g = [{"log_size": 3, "d_cols": z(1, 2, 8), "n_cols": 2}]
    q = {"groups": g, "gp": [[(0, 2)]], "b": 1, "pts": z(1, 1, 8), "np": 1, "samples": z(1, 1, 2, 4), "after": z(1, 4), "quot": mark(1, 4 * 16),
         "source": 0}

    def q_refused(code, **kw):
        a = dict(q, **kw)
        with pytest.raises(rsv.RsvError) as e:
            ctx.fri_quotients(a["groups"], a["gp"], 1, a["b"], a["pts"], a["np"], a["samples"], a["after"], a["quot"], source=a["source"])
        assert e.value.code == code, (code, e.value.code, kw)

    for k in ("pts", "samples", "after", "quot"):
        q_refused(-1, **{k: None})
    q_refused(-1, groups=[dict(g[0], d_cols=None)])
    q_refused(-2, b=0)
    q_refused(-2, b=17)
    q_refused(-2, np=0)
    q_refused(-2, np=5)
    q_refused(-2, source=2)
    q_refused(-2, gp=[[(0, 3)]])
    q_refused(-2, groups=[dict(g[0], log_size=0)])
    q_refused(-2, groups=[dict(g[0], log_size=30)])
    q_refused(-2, groups=g * 9, gp=[[(0, 2)]] * 9)
    q_refused(-2, pts=raw[1:33])
    q_refused(-2, quot=raw[2:258])
    # commit: one column of size 4, blowup 1, log_last 1
    c = {"quot": z(1, 64), "sizes": [4], "b": 1, "last": 1, "chan": mark(1, 16), "roots": mark(1, 2, 8), "alphas": mark(1, 2, 4),
         "layers": mark(1, 32), "poly": mark(1, 2, 4), "low": torch.full((1,), 7, dtype=torch.uint8, device=dev)}

    def c_refused(code, **kw):
        a = dict(c, **kw)
        with pytest.raises(rsv.RsvError) as e:
            ctx.fri_commit(a["quot"], a["sizes"], a["b"], a["last"], 1, a["chan"], a["roots"], a["alphas"], a["layers"], a["poly"], a["low"])
        assert e.value.code == code, (code, e.value.code, kw)

    for k in ("quot", "chan", "roots", "alphas", "layers", "poly", "low"):
        c_refused(-1, **{k: None})
    c_refused(-2, sizes=[4, 4])
    c_refused(-2, sizes=[4, 5])
    c_refused(-2, sizes=[31])
    c_refused(-2, sizes=[4, 2])   # a column of log size 1 <= log_last
    c_refused(-2, last=3)
    c_refused(-2, sizes=[30], last=17)
    c_refused(-2, b=0)
    c_refused(-2, roots=raw[1:65])
    ctx.synchronize()
    for k in ("chan", "roots", "alphas", "layers", "poly"):
        assert bool((c[k] == 0x5A5A5A5A).all()), k
    assert bool((q["quot"] == 0x5A5A5A5A).all()) and int(c["low"][0]) == 7
    ctx.close()
