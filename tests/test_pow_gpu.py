"""rsv_pow_grind_dev / rsv_draw_queries_dev / Chain.pow / Chain.open (`-m gpu`): the proof-of-work nonce and the queries of
the next proof, and the openings of trees 0-3 at them.  Against the REFERENCE for all 14 consecutive fixture pairs (the chain
of fixture K, given K+1's log_blowup, log_last, pow_bits and n_queries and nothing else, finds K+1's stored nonce, its
proof-of-work digest, its query positions, and its queried_values[0..3] and hash_witness[0..3]), bit for bit against the
numpy restatement (tests/pow_ref.py, pinned to the reference by tests/test_pow_host.py) on random channels where the search
changes shape, the cap on the candidates, the draw, and the refusals.  Every comparison is exact on 32-bit words; outputs are
prefilled with 0xffffffff."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import oracle_binding as ob
from tests import pow_ref as W
from tests.chain_harness import DEV, chain, dev, full, inputs_of, mask_dev, masked_past_64, pin_id, pins, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = C.P


# ---------------------------------------------------------------- the fixture pairs
def _cut(values, n_values, witness, n_witness):
    """One tree of one proof -> (values, witness nodes) cut at the counts; the words past them are zero."""
    assert n_values <= len(values) and n_witness <= len(witness)
    assert not values[n_values:].any() and not witness[n_witness:].any()
    return values[:n_values], witness[:n_witness]


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_chain_finds_the_next_fixtures_nonce_queries_and_openings(rsv, pin):
    """Chain.pow and Chain.open of fixture K: K+1's stored nonce (the smallest from 0), the digest behind its mix
    (transcript_raw words 32..39; the draws leave the digest alone), the query positions, and for trees 0-3 K+1's
    queried_values and hash_witness in count and word for word, zero past the counts."""
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    cfg = fixture_cfg(dst)
    b, nq = cfg.log_blowup_factor, cfg.n_queries
    nxt = read_proof(dst)
    ctx = rsv.Context(0)
    ch = chain(rsv, ctx, wp, [read_proof(src)], inputs_of(src), b, upto="fri", caps=True, log_last=cfg.log_last_layer_degree_bound)
    ch.pow(cfg.pow_bits, nq)
    ch.open()
    got = ch.numpy()
    vcaps, _ = rsv.witness_decommit_sizes(wp, b, nq)
    top = max(wp.trace_sizes()) + b
    ctx.close()
    wp.close()
    nonce = int(got["nonce"][0, 0]) | int(got["nonce"][0, 1]) << 32
    print(f"{src} -> {dst}: pow_bits {cfg.pow_bits}, nonce {nonce}, stored {W.stored_nonce(nxt, ob)}")
    assert got["ok"].tolist() == [1]
    assert nonce == W.stored_nonce(nxt, ob)
    tr = ob.transcript_raw(nxt)
    assert np.array_equal(got["channel"][0, :8], tr[32:40].astype(np.uint32))
    assert got["channel"][0, 8] == (nq + 7) // 8 and not got["channel"][0, 9:].any()
    qM, M = C.query_positions(nxt, ob)
    assert got["queries"].shape == (1, nq) and np.array_equal(got["queries"][0].astype(np.int64), qM)
    assert np.array_equal(got["queries_low"][0].astype(np.int64), qM >> (M - top))
    want = ob.split_variable_part(nxt)
    off = 0
    for t in range(4):
        if t < 3:
            vals, wit = _cut(got["values"][0, off:off + vcaps[t]], got["n_values"][0, t], got["witness_nodes"][0, t], got["n_witness"][0, t])
            off += vcaps[t]
        else:
            vals, wit = _cut(got["values3"][0], got["n_values3"][0], got["witness3"][0], got["n_witness3"][0])
        wv = np.array([int(x) for x in want["queried_values"][t]], np.uint32)
        ww = np.array(want["hash_witness"][t], np.uint32).reshape(-1, 8)
        assert len(vals) == len(wv) and np.array_equal(vals, wv), t
        assert len(wit) == len(ww) and np.array_equal(wit, ww), t


# ---------------------------------------------------------------- the search on random channels
def _channels(seeds):
    """uint32[n, 16]: a random canonical digest per seed, n_sent as a mix never leaves it (the mix resets it), zeros."""
    out = np.zeros((len(seeds), 16), np.uint32)
    for k, s in enumerate(seeds):
        rng = np.random.default_rng(s)
        out[k, :8] = rng.integers(0, P, 8)
        out[k, 8] = rng.integers(1, 5)
    return out


def _grind(ctx, chans, pow_bits, start=0, max_tries=0, mask=None):
    import torch
    n = len(chans)
    d_chan, d_nonce = dev(chans), full((n, 2))
    d_ok = torch.ones(n, dtype=torch.uint8, device=torch.device(DEV)) if mask is None else mask_dev(mask)
    ctx.pow_grind(pow_bits, n, d_ok, d_chan, d_nonce, start=start, max_tries=max_tries)
    ctx.synchronize()
    nonce = u32(d_nonce).astype(np.uint64)
    return [int(lo) | int(hi) << 32 for lo, hi in nonce], u32(d_chan), d_ok.cpu().numpy()


def _check_grind(ctx, chans, pow_bits, start=0, mask=None, beyond=None):
    """The device against the restatement, proof by proof; beyond: every restated nonce is at or past it (what the seeds
    were chosen for) -> the restated nonces."""
    limit = 1 << (pow_bits + 6)
    want = [W.grind(c, pow_bits, start, limit, ob) for c in chans]
    assert all(w is not None for w in want)
    if beyond is not None:
        assert all(w >= beyond for w in want), (want, beyond)
    nonce, after, ok = _grind(ctx, chans, pow_bits, start=start, mask=mask)
    for p, c in enumerate(chans):
        if mask is not None and not mask[p]:
            assert nonce[p] == 0 and not after[p].any() and ok[p] == 0, p
            continue
        assert nonce[p] == want[p], (p, nonce[p], want[p])
        assert np.array_equal(after[p], W.mix_nonce(c, want[p], ob)) and ok[p] == 1, p
    return want


# (pow_bits, start, seeds, the restated nonces lie at or past).  The seeds are fixed so that the search has to go where the
# case says: past the first round of 2^pow_bits lanes, or across the boundary of a nonce word.
GRIND = {
    "pow_bits_0": (0, 0, (1, 2), None),
    "pow_bits_0_from_a_start": (0, 12345, (1,), 12345),
    "pow_bits_1_smallest_of_many": (1, 0, (1, 2, 3), None),
    "pow_bits_4_smallest_of_many": (4, 0, (1, 2, 3), None),
    "pow_bits_12_rounds_beyond_the_first": (12, 0, (3, 5), 2 << 12),
    "pow_bits_17_rounds_beyond_the_first": (17, 0, (4,), 2 << 17),
    "into_the_second_word": (8, (1 << 22) - 64, (5, 8), 1 << 22),
    "into_the_third_word": (12, (1 << 43) - 64, (1, 2), 1 << 43),
}


@pytest.mark.parametrize("case", list(GRIND))
def test_grind_bit_for_bit(rsv, case):
    pow_bits, start, seeds, beyond = GRIND[case]
    ctx = rsv.Context(0)
    want = _check_grind(ctx, _channels(seeds), pow_bits, start=start, beyond=beyond)
    ctx.close()
    if pow_bits == 0:
        assert want == [start] * len(seeds)


def test_batch_of_five_with_a_masked_proof(rsv):
    ctx = rsv.Context(0)
    _check_grind(ctx, _channels((11, 12, 13, 14, 15)), 9, mask=[1, 1, 0, 1, 1])
    ctx.close()


def test_grind_past_one_workgroup_of_proofs(rsv):
    """70 channels at pow_bits 4, proofs 63 and 64 masked: k_pow_finish's second workgroup of proofs, every proof against the
    restatement."""
    ctx = rsv.Context(0)
    _check_grind(ctx, _channels(range(100, 170)), 4, mask=masked_past_64())
    ctx.close()


def test_the_cap_on_the_candidates(rsv):
    """max_tries = k + 1 finds the nonce k, max_tries = k exhausts: ok cleared, zero nonce, zeroed channel; the neighbour,
    whose nonce is smaller, is found either way."""
    chans = _channels((21, 22))
    k, k1 = (W.grind(c, 8, 0, 1 << 14, ob) for c in chans)
    if k < k1:
        chans, k, k1 = chans[::-1].copy(), k1, k
    assert k1 < k
    ctx = rsv.Context(0)
    nonce, after, ok = _grind(ctx, chans, 8, max_tries=k + 1)
    assert nonce == [k, k1] and ok.tolist() == [1, 1]
    assert np.array_equal(after[0], W.mix_nonce(chans[0], k, ob)) and np.array_equal(after[1], W.mix_nonce(chans[1], k1, ob))
    nonce, after, ok = _grind(ctx, chans, 8, max_tries=k)
    ctx.close()
    assert nonce == [0, k1] and ok.tolist() == [0, 1]
    assert not after[0].any() and np.array_equal(after[1], W.mix_nonce(chans[1], k1, ob))


# ---------------------------------------------------------------- the draw
def _check_draw(ctx, chans, mask, nq, log_size, log_low):
    """With and without the low positions: the queries, the low queries, n_sent; zeros for a masked proof."""
    n = len(chans)
    for with_low in (True, False):
        d_chan, d_q, d_low = dev(chans), full((n, nq)), full((n, nq))
        ctx.draw_queries(n, nq, log_size, log_low, d_chan, d_q, d_low if with_low else None, d_mask=mask_dev(mask))
        ctx.synchronize()
        after, q, low = u32(d_chan), u32(d_q), u32(d_low)
        for p in range(n):
            if not mask[p]:
                assert not after[p].any() and not q[p].any()
                assert not low[p].any() if with_low else (low[p] == 0xFFFFFFFF).all()
                continue
            wq, wlow, wafter = W.draw_queries(chans[p], nq, log_size, log_low, ob)
            assert np.array_equal(q[p], wq) and np.array_equal(after[p], wafter), p
            assert wafter[8] == chans[p, 8] + (nq + 7) // 8
            assert np.array_equal(low[p], wlow) if with_low else (low[p] == 0xFFFFFFFF).all(), p


@pytest.mark.parametrize("nq,log_size,log_low", [(1, 1, 1), (8, 20, 20), (9, 20, 13), (128, 30, 30), (128, 30, 7), (9, 30, 1)])
def test_draw_bit_for_bit(rsv, nq, log_size, log_low):
    """Three proofs, the second masked, with and without the low positions: the queries, the low queries, n_sent."""
    chans = _channels((31, 32, 33))
    chans[:, 8] = (0, 0, 2)
    ctx = rsv.Context(0)
    _check_draw(ctx, chans, [1, 0, 1], nq, log_size, log_low)
    ctx.close()


def test_draw_past_one_workgroup_of_proofs(rsv):
    """70 proofs, 63 and 64 masked: k_pow_queries' second workgroup of proofs, every proof against the restatement."""
    ctx = rsv.Context(0)
    _check_draw(ctx, _channels(range(200, 270)), masked_past_64(), 9, 20, 13)
    ctx.close()


# ---------------------------------------------------------------- refusals
def test_device_refusals(rsv):
    """NULL pointers, sizes and misalignment with a live context: the neighbours' codes, nothing written."""
    import torch
    device = torch.device(DEV)
    ctx = rsv.Context(0)
    raw = torch.zeros(8192, dtype=torch.uint8, device=device)
    mark = lambda *shape: torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=device)  # noqa: E731
    g = {"bits": 4, "start": 0, "tries": 0, "n": 1, "ok": torch.full((1,), 7, dtype=torch.uint8, device=device), "chan": mark(1, 16), "nonce": mark(1, 2)}

    def g_refused(code, **kw):
        a = dict(g, **kw)
        with pytest.raises(rsv.RsvError) as e:
            ctx.pow_grind(a["bits"], a["n"], a["ok"], a["chan"], a["nonce"], start=a["start"], max_tries=a["tries"])
        assert e.value.code == code, (code, e.value.code, kw)

    for k in ("ok", "chan", "nonce"):
        g_refused(-1, **{k: None})
    g_refused(-2, bits=31)
    g_refused(-2, n=0)
    g_refused(-2, n=(1 << 20) + 1)
    g_refused(-2, start=(1 << 64) - 1, tries=1)
    g_refused(-2, start=(1 << 64) - 16)          # the default 2^(4 + 6) candidates pass 2^64
    g_refused(-2, start=1, tries=(1 << 64) - 1)
    g_refused(-2, chan=raw[1:65])
    g_refused(-2, nonce=raw[2:10])
    d = {"n": 1, "nq": 8, "log": 10, "low": 5, "chan": mark(1, 16), "q": mark(1, 8), "qlow": mark(1, 8)}

    def d_refused(code, **kw):
        a = dict(d, **kw)
        with pytest.raises(rsv.RsvError) as e:
            ctx.draw_queries(a["n"], a["nq"], a["log"], a["low"], a["chan"], a["q"], a["qlow"])
        assert e.value.code == code, (code, e.value.code, kw)

    for k in ("chan", "q"):
        d_refused(-1, **{k: None})
    d_refused(-2, n=0)
    d_refused(-2, n=(1 << 20) + 1)
    d_refused(-2, nq=0)
    d_refused(-2, nq=129)
    d_refused(-2, low=0)
    d_refused(-2, low=11)
    d_refused(-2, log=31, low=31)
    d_refused(-2, chan=raw[1:65])
    d_refused(-2, q=raw[2:34])
    d_refused(-2, qlow=raw[3:35])
    ctx.synchronize()
    for k in ("chan", "nonce"):
        assert bool((g[k] == 0x5A5A5A5A).all()), k
    for k in ("chan", "q", "qlow"):
        assert bool((d[k] == 0x5A5A5A5A).all()), k
    assert int(g["ok"][0]) == 7
    ctx.close()
