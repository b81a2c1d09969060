"""rsv_fri_commit_tail_dev / rsv_witness_fri_tail_dev / Chain(fri_tail_log=t) (`-m gpu`): the commit phase of FRI with the top
of every layer tree, and the small layers with the last one, finished by one workgroup per proof.  On random quotient columns,
bit for bit against the numpy restatement (tests/fri_ref.py) and against a tail_log = 0 run of the same inputs, at the smallest
shapes where a path changes: t below, on and above the last layer's size, a column joining before and inside the tail, a first
tree that lies wholly under t, a level strided over the workgroup; with the caps kept; batches with masked proofs and proofs
cut into passes; both values of low_degree; the refusals; and against the REFERENCE for all 14 consecutive fixture pairs: the
chain of fixture K in the tail form puts out fixture K+1's file.  Every comparison is exact on 32-bit words; outputs and d_caps
are prefilled with 0xffffffff, which no M31 word equals."""
import functools

import numpy as np
import pytest

from tests import commit_ref as C
from tests import fri_ref as F
from tests import oracle_binding as ob
from tests.chain_harness import DEV, FILL, dev, full, inputs_of, mask_dev, masked_past_64, pin_id, pin_of, pins, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = C.P
OUTPUTS = ("roots", "alphas", "layers", "last", "low", "chan")


def _columns(seed, sizes, n=1):
    rng = np.random.default_rng(seed)
    return [{s: rng.integers(0, P, (4, 1 << s)) for s in sizes} for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _restated(seed, sizes, log_last, b, p=0, n=1):
    """The restatement's commitment of proof p of _columns(seed, sizes, n), computed once per shape -> (outputs, the channel)."""
    ch = C.Channel(ob, np.zeros(8, np.uint32), 0)
    return F.commit(_columns(seed, sizes, n)[p], log_last, b, ch, ob), ch


def _run(rsv, ctx, sizes, log_last, b, cols, t, h=0, mask=None):
    """cols: per proof {size: (4, 2^size)} -> the numpy outputs of Context.fri_commit(tail_log=t, sub_log=h)."""
    import torch
    sizes, n = list(sizes), len(cols)
    ni = F.n_inner_of(sizes[0], log_last, b)
    lw = sum(4 << (sizes[0] - 1 - i) for i in range(ni))
    quot = dev(np.stack([np.concatenate([c[s].reshape(-1) for s in sizes]) for c in cols]))
    chan = dev(np.zeros((n, 16), np.uint32))
    roots, alphas, layers, last = full((n, 1 + ni, 8)), full((n, 1 + ni, 4)), full((n, max(lw, 1))), full((n, 1 << log_last, 4))
    low = torch.full((n,), 7, dtype=torch.uint8, device=torch.device(DEV))
    words, caps = 0, None
    if h:
        words = rsv.fri_cap_sizes(sizes, b, log_last, h, n)[0]
        caps = full((max(words, 1),))
    ctx.fri_commit(quot, sizes, b, log_last, n, chan, roots, alphas, layers if ni else None, last, low, d_mask=mask_dev(mask), sub_log=h, d_caps=caps,
                   tail_log=t)
    ctx.synchronize()
    got = dict(roots=u32(roots), alphas=u32(alphas), layers=u32(layers)[:, :lw], last=u32(last), chan=u32(chan), low=low.cpu().numpy())
    if h:
        got["caps"] = u32(caps)[:words]
    return got, (quot, layers if ni else None, caps)


def _same(got, ref, keys=OUTPUTS):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), k


def _check_proof(got, p, want, ch):
    assert np.array_equal(got["roots"][p], want["roots"]) and np.array_equal(got["alphas"][p], want["alphas"]), p
    assert np.array_equal(got["last"][p], want["last_poly"]), p
    print(f"proof {p}: low_degree {got['low'][p]} (want {want['low_degree']})")
    assert got["low"][p] == want["low_degree"], p
    if want["layers"]:
        assert np.array_equal(got["layers"][p], np.concatenate([np.asarray(ev).reshape(-1) for ev in want["layers"]]).astype(np.uint32)), p
    assert np.array_equal(got["chan"][p, :8], ch.digest) and got["chan"][p, 8] == ch.n_sent and not got["chan"][p, 9:].any(), p


# (sizes, log_last, b, t): [7,6,5] has L = 3 and the inner layers 6, 5, 4 — t 2: t < L, tree tops only; 3: the tail is the last
# layer only; 4: column 5 joins in the hand-off fold; 5: inside the tail; 6: every inner layer in the tail, tree 0's top carries
# the columns at levels 6 and 5; 7: the whole first tree in k_fr_tree_top.  [4]: no inner layer.  [11,9]: t 10 strides a level of
# 1 024 nodes and joins column 9 in the tail, t 8 joins it outside.
SHAPES = [((7, 6, 5), 2, 1, t) for t in (2, 3, 4, 5, 6, 7)] + [((4,), 2, 1, 3), ((4,), 2, 1, 4), ((11, 9), 1, 1, 10), ((11, 9), 1, 1, 8)]


@pytest.mark.parametrize("sizes,log_last,b,t", SHAPES, ids=["-".join(map(str, s)) + f"-t{t}" for s, _, _, t in SHAPES])
def test_tail_form_bit_for_bit(rsv, sizes, log_last, b, t):
    """Random columns through tail_log = t: the restatement's outputs, and the tail_log = 0 run's word for word."""
    seed = 2700 + len(sizes) + sizes[0]
    cols = _columns(seed, sizes)
    ctx = rsv.Context(0)
    got, _ = _run(rsv, ctx, sizes, log_last, b, cols, t)
    ref, _ = _run(rsv, ctx, sizes, log_last, b, cols, 0)
    ctx.close()
    for k in OUTPUTS:
        assert not (got[k] == FILL).any(), k
    _same(got, ref)
    _check_proof(got, 0, *_restated(seed, sizes, log_last, b))


@pytest.mark.parametrize("h,t", [(2, 6), (1, 4), (3, 2)], ids=["h2-t6", "h1-t4", "h3-t2"])
def test_tail_form_leaves_the_caps(rsv, h, t):
    """[7,6,5] with the caps kept: no prefill word is left in d_caps, the caps are the per-layer form's, and fri_open from them
    gives the lists it gives from the per-layer form's."""
    sizes, log_last, b, nq = (7, 6, 5), 2, 1, 16
    seed = 2710
    cols = _columns(seed, sizes)
    queries = dev(np.random.default_rng(seed).integers(0, 1 << sizes[0], (1, nq)).astype(np.int64))
    vcap, wcap = rsv.fri_open_sizes(list(sizes), b, log_last, nq)
    ctx = rsv.Context(0)
    lists = []
    runs = []
    for tail in (t, 0):
        got, (quot, layers, caps) = _run(rsv, ctx, sizes, log_last, b, cols, tail, h=h)
        out = {"fw": full((1, 4, vcap, 4)), "nf": full((1, 4)), "hw": full((1, 4, wcap, 8)), "nh": full((1, 4))}
        ctx.fri_open(quot, layers, list(sizes), b, log_last, 1, queries, nq, out["fw"], out["nf"], out["hw"], out["nh"], sub_log=h, d_caps=caps)
        ctx.synchronize()
        runs.append(got)
        lists.append({k: u32(v) for k, v in out.items()})
    ctx.close()
    got, ref = runs
    assert got["caps"].size and not (got["caps"] == FILL).any()
    _same(got, ref, OUTPUTS + ("caps",))
    for k in lists[0]:
        assert np.array_equal(lists[0][k], lists[1][k]), k
    _check_proof(got, 0, *_restated(seed, sizes, log_last, b))


def test_batch_with_a_masked_proof(rsv):
    """Three proofs with their own columns, the middle one masked: zeros in its roots, alphas, channel, layers and last
    polynomial, low_degree 0; its neighbours the restatement's."""
    sizes, log_last, b, seed = (7, 6, 5), 2, 1, 2720
    cols = _columns(seed, sizes, 3)
    ctx = rsv.Context(0)
    got, _ = _run(rsv, ctx, sizes, log_last, b, cols, 6, mask=[1, 0, 1])
    ref, _ = _run(rsv, ctx, sizes, log_last, b, cols, 0, mask=[1, 0, 1])
    ctx.close()
    _same(got, ref)
    for k in ("roots", "alphas", "chan", "layers", "last"):
        assert not got[k][1].any(), k
    assert got["low"][1] == 0
    for p in (0, 2):
        _check_proof(got, p, *_restated(seed, sizes, log_last, b, p, 3))


def test_past_one_workgroup_of_proofs(rsv):
    """70 proofs of [4], 2, 1 with their own columns, 63 and 64 masked."""
    sizes, log_last, b, seed, n = (4,), 2, 1, 2730, 70
    mask = masked_past_64()
    cols = _columns(seed, sizes, n)
    ctx = rsv.Context(0)
    got, _ = _run(rsv, ctx, sizes, log_last, b, cols, 4, mask=mask)
    ref, _ = _run(rsv, ctx, sizes, log_last, b, cols, 0, mask=mask)
    ctx.close()
    _same(got, ref)
    for p in range(n):
        if not mask[p]:
            assert all(not got[k][p].any() for k in ("roots", "alphas", "chan", "last")) and got["low"][p] == 0, p
        else:
            _check_proof(got, p, *_restated(seed, sizes, log_last, b, p, n))


def test_commit_cut_into_passes(rsv):
    """Five proofs of [13,11], 9, 1 under a 1 MB budget, t 10: L = 10 is the largest last layer the tail takes.  The two node
    layers of three proofs exceed the budget, so the proofs take at least three passes; the cut run equals the uncut run in every
    output and in the caps, and one proof of the last pass the restatement."""
    sizes, log_last, b, n, t, h, seed = (13, 11), 9, 1, 5, 10, 8, 2740
    budget, node_bytes = 1 << 20, 48 << sizes[0]
    assert 3 * node_bytes > budget >= 2 * node_bytes
    cols = _columns(seed, sizes, n)
    ctx = rsv.Context(0)
    whole, _ = _run(rsv, ctx, sizes, log_last, b, cols, t, h=h)
    ctx.set_option("ws_budget_mb", 1)
    cut, _ = _run(rsv, ctx, sizes, log_last, b, cols, t, h=h)
    ctx.close()
    assert whole["caps"].size and not (whole["caps"] == FILL).any()
    _same(cut, whole, OUTPUTS + ("caps",))
    _check_proof(cut, 4, *_restated(seed, sizes, log_last, b, 4, n))


def test_both_values_of_low_degree(rsv):
    """Random columns leave non-zero coefficients past 2^log_last: low_degree 0.  Constant columns are polynomials of degree 0:
    every fold of a constant is a constant, the last layer's polynomial is its first coefficient alone: low_degree 1."""
    sizes, log_last, b, seed = (7, 6, 5), 2, 1, 2750
    rng = np.random.default_rng(seed)
    flat = {s: np.repeat(rng.integers(1, P, (4, 1)), 1 << s, axis=1) for s in sizes}
    ch = C.Channel(ob, np.zeros(8, np.uint32), 0)
    want = F.commit(flat, log_last, b, ch, ob)
    assert want["low_degree"] == 1 and want["last_poly"][0].any() and not want["last_poly"][1:].any()
    ctx = rsv.Context(0)
    seen = set()
    for t in (3, 6):
        got, _ = _run(rsv, ctx, sizes, log_last, b, [flat], t)
        _check_proof(got, 0, want, ch)
        rand, _ = _run(rsv, ctx, sizes, log_last, b, _columns(seed, sizes), t)
        _check_proof(rand, 0, *_restated(seed, sizes, log_last, b))
        seen |= {int(got["low"][0]), int(rand["low"][0])}
    ctx.close()
    assert seen == {0, 1}


def test_device_refusals(rsv):
    """tail_log 11 is refused after everything the cap form refuses, in its order; nothing is written."""
    import torch
    device = torch.device(DEV)
    ctx = rsv.Context(0)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)  # noqa: E731
    raw = torch.zeros(8192, dtype=torch.uint8, device=device)
    mark = lambda *shape: torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=device)  # noqa: E731
    words, _ = rsv.fri_cap_sizes([5], 1, 1, 2)
    c0 = {"quot": z(1, 128), "sizes": [5], "b": 1, "last": 1, "chan": mark(1, 16), "roots": mark(1, 3, 8), "alphas": mark(1, 3, 4),
          "layers": mark(1, 96), "poly": mark(1, 2, 4), "low": torch.full((1,), 7, dtype=torch.uint8, device=device), "h": 2, "caps": mark(words), "t": 4}

    def refused(code, **kw):
        a = dict(c0, **kw)
        with pytest.raises(rsv.RsvError) as e:
            ctx.fri_commit(a["quot"], a["sizes"], a["b"], a["last"], 1, a["chan"], a["roots"], a["alphas"], a["layers"], a["poly"], a["low"],
                           sub_log=a["h"], d_caps=a["caps"], tail_log=a["t"])
        assert e.value.code == code, (code, e.value.code, kw)

    refused(-2, t=11)
    refused(-2, t=11, caps=None, h=0)
    for k in ("quot", "chan", "roots", "alphas", "layers", "poly", "low"):
        refused(-1, **{k: None})
        refused(-1, **{k: None}, t=11)  # a NULL comes before tail_log
    refused(-1, roots=None, h=0)
    refused(-2, sizes=[5, 6])
    refused(-2, last=4)
    refused(-2, h=0)
    refused(-2, h=9)
    refused(-2, caps=raw[1:1 + 4 * words])
    refused(-2, chan=raw[2:66])
    ctx.synchronize()
    for k in ("chan", "roots", "alphas", "layers", "poly", "caps"):
        assert bool((c0[k] == 0x5A5A5A5A).all()), k
    assert int(c0["low"][0]) == 7
    ctx.close()


# ---------------------------------------------------------------- the fixture pairs
def _tail_chain(rsv, ctx, wp, pin, fri_caps=True):
    src, cfg = pin["src"], fixture_cfg(pin["dst"])
    ch = rsv.Chain(ctx, wp, 1, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, fri_sub_log=8 if fri_caps else 0,
                   fri_tail_log=10, device=DEV)
    ch.witness([read_proof(src)], inputs_of(src))
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch, stage)()
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.open()
    ch.fri_open()
    return ch


def _check_next_fixture(ch, dst):
    got, proofs = ch.numpy(), ch.proofs()
    want = ob.split_variable_part(read_proof(dst))["layers"]
    assert got["ok"].tolist() == [1] and got["low_degree"].tolist() == [1]
    assert got["fri_roots"].shape == (1, len(want), 8)
    for t, layer in enumerate(want):
        assert np.array_equal(got["fri_roots"][0, t], layer["commitment"]), t
    assert proofs[0] is not None and proofs[0] == read_proof(dst)
    return got


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_tail_chain_outputs_the_next_fixture(rsv, pin):
    """Chain(caps=True, fri_sub_log=8, fri_tail_log=10) of fixture K through pow, open, fri_open and proofs(): fixture K+1's
    file byte for byte, its fri_roots the stored commitments."""
    wp = program_of(rsv, pin)
    ctx = rsv.Context(0)
    ch = _tail_chain(rsv, ctx, wp, pin)
    assert ch.fri_tail_log == 10 and ch.fri_caps is not None
    got = _check_next_fixture(ch, pin["dst"])
    ctx.close()
    wp.close()
    assert not (got["fri_caps"] == FILL).any()


def test_tail_chain_packs_a_proof_the_verifier_accepts(rsv):
    """One pair through Chain.pack() into rsv_verify_batch_dev; and the same pair with fri_tail_log=10 and no caps of the
    layer trees."""
    import torch
    pin = pin_of("level1-5.bin")
    dst = pin["dst"]
    wp = program_of(rsv, pin)
    ctx = rsv.Context(0)
    ch = _tail_chain(rsv, ctx, wp, pin)
    d_blob, d_offsets = ch.pack()
    acc = torch.full((1,), 7, dtype=torch.uint8, device=DEV)
    reason = torch.full((1,), 77, dtype=torch.uint8, device=DEV)
    ctx.verify_batch(d_blob, d_offsets, 1, acc, reason, cfg=fixture_cfg(dst), inputs=inputs_of(dst))
    ctx.synchronize()
    assert (acc.cpu().tolist(), reason.cpu().tolist()) == ([1], [0])
    bare = _tail_chain(rsv, ctx, wp, pin, fri_caps=False)
    assert bare.fri_caps is None
    _check_next_fixture(bare, dst)
    ctx.close()
    wp.close()
