"""rsv_fri_commit_cap_dev / rsv_fri_open_cap_dev / Chain(fri_sub_log=h) (`-m gpu`): the commitment that keeps the top of every
FRI layer tree and the opening that rebuilds only the subtrees under it.  On random quotient columns, bit for bit against the
numpy restatement (tests/fri_ref.py, tests/fri_open_ref.py) at the smallest shapes where a path changes: the cap's lowest
layer on, above and below a data layer, a tree too small to keep anything, a subtree past one wave of leaves, the sibling
nobody queries; batches with masked proofs and with the commitment cut into passes; the refusals; and against the REFERENCE
for all 14 consecutive fixture pairs: the capped chain of fixture K puts out fixture K+1's file.  Every comparison is exact on
32-bit words; outputs and d_caps are prefilled with 0xffffffff, which no M31 word equals."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import fri_open_ref as FO
from tests import fri_ref as F
from tests import oracle_binding as ob
from tests.chain_harness import DEV, FILL, dev, full, inputs_of, mask_dev, masked_past_64, pin_id, pin_of, pins, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = C.P

# (sizes, log_last, b) of tests/test_fri_open_gpu.py's SHAPES, and the pair of the sibling-subtree example
SHAPES = {
    "three_columns": ([7, 6, 5], 2, 1),
    "no_inner_layer": ([4], 2, 1),
    "levels_past_one_workgroup": ([11, 9], 1, 1),
    "sibling_subtree": ([7, 4], 1, 1),
    "width_256": ([9, 8, 6], 1, 1),
}


def _run(rsv, ctx, sizes, log_last, b, h, cols, queries, mask=None):
    """cols: per proof {size: (4, 2^size)}; queries [n][nq] -> the numpy outputs of the capped fri_commit (roots, alphas,
    layers, last, low, chan, caps) and of the capped fri_open (fw [n, T, vcap, 4], nf [n, T], hw [n, T, wcap, 8], nh [n, T])."""
    import torch
    n, nq = len(cols), len(queries[0])
    ni = F.n_inner_of(sizes[0], log_last, b)
    T = 1 + ni
    lw = sum(4 << (sizes[0] - 1 - i) for i in range(ni))
    quot = np.stack([np.concatenate([c[s].reshape(-1) for s in sizes]) for c in cols])
    chan = dev(np.zeros((n, 16), np.uint32))
    roots, alphas, layers, last = full((n, T, 8)), full((n, T, 4)), full((n, max(lw, 1))), full((n, 1 << log_last, 4))
    low = torch.full((n,), 7, dtype=torch.uint8, device=torch.device(DEV))
    words, trees = rsv.fri_cap_sizes(sizes, b, log_last, h, n)
    caps = full((max(words, 1),))
    d_mask, d_quot, d_queries = mask_dev(mask), dev(quot), dev(np.asarray(queries, dtype=np.int64))
    ctx.fri_commit(d_quot, sizes, b, log_last, n, chan, roots, alphas, layers if ni else None, last, low, d_mask=d_mask, sub_log=h, d_caps=caps)
    vcap, wcap = rsv.fri_open_sizes(sizes, b, log_last, nq)
    out = {"fw": full((n, T, vcap, 4)), "nf": full((n, T)), "hw": full((n, T, wcap, 8)), "nh": full((n, T))}
    ctx.fri_open(d_quot, layers if ni else None, sizes, b, log_last, n, d_queries, nq, out["fw"], out["nf"], out["hw"], out["nh"], d_mask=d_mask,
                 sub_log=h, d_caps=caps)
    ctx.synchronize()
    got = {k: u32(v) for k, v in out.items()}
    got.update(roots=u32(roots), alphas=u32(alphas), layers=u32(layers), last=u32(last), chan=u32(chan), low=low.cpu().numpy(),
               caps=u32(caps)[:words], trees=np.array(trees, np.int64))
    return got


def _check_proof(got, p, n, sizes, log_last, b, h, cols, queries):
    """Proof p of a run of n against the restatement on the restated commitment: the commitment's outputs, the kept layers,
    both lists of every tree, and the consumer's walk of the device's lists back to the device's roots."""
    M = sizes[0]
    ch = C.Channel(ob, np.zeros(8, np.uint32), 0)
    want = F.commit(cols, log_last, b, ch, ob)
    nodes = []
    opened = FO.open_all(cols, want["layers"], queries, ob, node_cache=nodes)
    assert got["nf"].shape[1] == len(opened)
    assert np.array_equal(got["roots"][p], want["roots"]) and np.array_equal(got["alphas"][p], want["alphas"]), p
    assert np.array_equal(got["last"][p], want["last_poly"]) and got["low"][p] == want["low_degree"], p
    if want["layers"]:
        assert np.array_equal(got["layers"][p], np.concatenate([np.asarray(ev).reshape(-1) for ev in want["layers"]]).astype(np.uint32)), p
    assert np.array_equal(got["chan"][p, :8], ch.digest) and got["chan"][p, 8] == ch.n_sent and not got["chan"][p, 9:].any(), p
    for t, ((top, layers), (fw, hw, root)) in enumerate(zip(FO.trees(cols, want["layers"]), opened)):
        c = max(top - h, 0)
        for l in range(1, c + 1):
            at = int(got["trees"][t]) + n * 8 * ((1 << l) - 2) + p * (8 << l)
            assert np.array_equal(got["caps"][at:at + (8 << l)].reshape(-1, 8), nodes[t][l]), (p, t, l)
        nf, nh = int(got["nf"][p, t]), int(got["nh"][p, t])
        print(f"proof {p} tree {t} (top {top}, kept layers {c}): fri_witness {nf} (want {len(fw)}), hash_witness {nh} (want {len(hw)})")
        assert (nf, nh) == (len(fw), len(hw)), (p, t)
        assert np.array_equal(got["fw"][p, t, :nf], fw) and np.array_equal(got["hw"][p, t, :nh], hw), (p, t)
        assert not got["fw"][p, t, nf:].any() and not got["hw"][p, t, nh:].any(), (p, t)
        assert np.array_equal(got["roots"][p, t], root), (p, t)
        qs = [(int(q) & ((1 << M) - 1)) >> (M - top) for q in queries]
        walked = FO.walk(got["fw"][p, t, :nf], got["hw"][p, t, :nh], qs, lambda l, x: layers[l][:, x], top, set(layers), ob)
        assert np.array_equal(walked, got["roots"][p, t]), (p, t)


def _sixteen(rng, M):
    """16 positions with duplicates and with both halves of a pair (at the leaves and one level up)."""
    q = rng.integers(0, 1 << M, 16)
    q[1], q[2], q[3], q[9] = q[0], q[0] ^ 1, q[5] ^ 2, q[8]
    return q.tolist()


# (shape, h, queries): with top = 7 in tree 0 of three_columns, h 1 puts the cap's lowest layer c on the data layer 6, h 2 on the
# data layer 5, h 3 on layer 4 just under the data layers, h 8 keeps nothing in any tree
CASES = [
    ("three_columns", 1, "sixteen"), ("three_columns", 2, "sixteen"), ("three_columns", 3, "sixteen"), ("three_columns", 8, "sixteen"),
    ("three_columns", 1, "one_query"),
    ("sibling_subtree", 3, "query_0"), ("sibling_subtree", 3, "sixteen"),
    ("no_inner_layer", 4, "sixteen"), ("no_inner_layer", 8, "sixteen"), ("no_inner_layer", 2, "every_position"),
    ("levels_past_one_workgroup", 8, "sixteen"), ("levels_past_one_workgroup", 2, "sixteen"),
    ("width_256", 3, "distinct_128"),
]


@pytest.mark.parametrize("shape,h,kind", CASES, ids=[f"{s}-h{h}-{k}" for s, h, k in CASES])
def test_capped_commit_and_open_bit_for_bit(rsv, shape, h, kind):
    """Random quotient columns through the capped commitment and the capped opening, against the restatement; no prefill word
    is left anywhere in d_caps."""
    sizes, log_last, b = SHAPES[shape]
    rng = np.random.default_rng(2600 + CASES.index((shape, h, kind)))
    M = sizes[0]
    cols = {s: rng.integers(0, P, (4, 1 << s)) for s in sizes}
    if kind == "one_query":
        queries = [int(rng.integers(0, 1 << M)) | 1 << 31]  # bits above M are ignored
    elif kind == "query_0":
        queries = [0]
    elif kind == "sixteen":
        queries = _sixteen(rng, M)
    elif kind == "every_position":
        queries = rng.permutation(1 << M).tolist()
    else:
        queries = rng.choice(1 << M, 128, replace=False).tolist()
    ctx = rsv.Context(0)
    got = _run(rsv, ctx, sizes, log_last, b, h, [cols], [queries])
    ctx.close()
    assert not (got["caps"] == FILL).any()
    _check_proof(got, 0, 1, sizes, log_last, b, h, cols, queries)
    if kind == "every_position":
        assert not got["nf"].any() and not got["nh"].any()
    if h == 8 and M <= 8:
        assert got["caps"].size == 0


def test_batch_with_a_masked_proof(rsv):
    """Three proofs with their own columns and queries, the middle one masked: zero counts and zero buffers for it, its
    neighbours' caps and openings the restatement's."""
    sizes, log_last, b = SHAPES["three_columns"]
    rng = np.random.default_rng(2630)
    cols = [{s: rng.integers(0, P, (4, 1 << s)) for s in sizes} for _ in range(3)]
    queries = [_sixteen(rng, sizes[0]) for _ in range(3)]
    ctx = rsv.Context(0)
    got = _run(rsv, ctx, sizes, log_last, b, 2, cols, queries, mask=[1, 0, 1])
    ctx.close()
    assert not (got["caps"] == FILL).any()
    for k in ("fw", "nf", "hw", "nh", "roots", "alphas", "chan"):
        assert not got[k][1].any(), k
    for p in (0, 2):
        _check_proof(got, p, 3, sizes, log_last, b, 2, cols[p], queries[p])


def test_past_one_workgroup_of_proofs(rsv):
    """70 proofs of the no_inner_layer shape with their own columns and four queries each, 63 and 64 masked."""
    sizes, log_last, b = SHAPES["no_inner_layer"]
    n, mask, h = 70, masked_past_64(), 2
    rng = np.random.default_rng(2650)
    cols = [{s: rng.integers(0, P, (4, 1 << s)) for s in sizes} for _ in range(n)]
    queries = [rng.integers(0, 1 << sizes[0], 4).tolist() for _ in range(n)]
    ctx = rsv.Context(0)
    got = _run(rsv, ctx, sizes, log_last, b, h, cols, queries, mask=mask)
    ctx.close()
    assert not (got["caps"] == FILL).any()
    for p in range(n):
        if not mask[p]:
            assert all(not got[k][p].any() for k in ("fw", "nf", "hw", "nh")), p
        else:
            _check_proof(got, p, n, sizes, log_last, b, h, cols[p], queries[p])


def test_commit_cut_into_passes_writes_the_cap_pass_by_pass(rsv):
    """Five proofs of 2^13 leaves under a 1 MB budget, h 8.  The commitment's two node layers are 48 x 2^M bytes a proof: those
    of three proofs exceed the budget, so the five proofs take at least three passes, each writing its own proofs of every kept
    layer.  d_caps and every output of the cut run equal the uncut run's, and one proof of the last pass the restatement's."""
    sizes, log_last, b, n, nq, h = [13, 11], 9, 1, 5, 4, 8
    budget, node_bytes = 1 << 20, 48 << sizes[0]
    assert 3 * node_bytes > budget >= 2 * node_bytes
    rng = np.random.default_rng(2640)
    cols = [{s: rng.integers(0, P, (4, 1 << s)) for s in sizes} for _ in range(n)]
    queries = [rng.integers(0, 1 << sizes[0], nq).tolist() for _ in range(n)]
    ctx = rsv.Context(0)
    whole = _run(rsv, ctx, sizes, log_last, b, h, cols, queries)
    ctx.set_option("ws_budget_mb", 1)
    cut = _run(rsv, ctx, sizes, log_last, b, h, cols, queries)
    ctx.close()
    assert whole["caps"].size and not (whole["caps"] == FILL).any()
    for k in whole:
        assert np.array_equal(cut[k], whole[k]), k
    _check_proof(whole, 4, n, sizes, log_last, b, h, cols[4], queries[4])


def test_defaults_make_the_old_calls_and_caps_off_recomputes(rsv):
    """With d_caps the opening equals the recompute form's, word for word, on the same commitment; Context.fri_commit with a
    sub_log and no d_caps is rsv_fri_commit_dev (nothing else to write)."""
    sizes, log_last, b = SHAPES["three_columns"]
    rng = np.random.default_rng(2660)
    cols = {s: rng.integers(0, P, (4, 1 << s)) for s in sizes}
    queries = _sixteen(rng, sizes[0])
    ctx = rsv.Context(0)
    capped = _run(rsv, ctx, sizes, log_last, b, 3, [cols], [queries])
    import torch
    ni, T = 3, 4
    quot = dev(np.concatenate([cols[s].reshape(-1) for s in sizes])[None])
    chan = dev(np.zeros((1, 16), np.uint32))
    roots, alphas, layers, last = full((1, T, 8)), full((1, T, 4)), full((1, sum(4 << (6 - i) for i in range(ni)))), full((1, 4, 4))
    low = torch.full((1,), 7, dtype=torch.uint8, device=torch.device(DEV))
    ctx.fri_commit(quot, sizes, b, log_last, 1, chan, roots, alphas, layers, last, low, sub_log=3, d_caps=None)
    vcap, wcap = rsv.fri_open_sizes(sizes, b, log_last, 16)
    out = {"fw": full((1, T, vcap, 4)), "nf": full((1, T)), "hw": full((1, T, wcap, 8)), "nh": full((1, T))}
    ctx.fri_open(quot, layers, sizes, b, log_last, 1, dev(np.asarray([queries], dtype=np.int64)), 16, out["fw"], out["nf"], out["hw"], out["nh"])
    ctx.synchronize()
    for k, v in out.items():
        assert np.array_equal(u32(v), capped[k]), k
    for k, v in (("roots", roots), ("alphas", alphas), ("layers", layers), ("last", last), ("chan", chan)):
        assert np.array_equal(u32(v), capped[k]), k
    ctx.close()


def test_device_refusals(rsv):
    """NULL pointers, sizes, sub_log and misalignment with a live context: the codes of the uncapped calls, nothing written."""
    import torch
    device = torch.device(DEV)
    ctx = rsv.Context(0)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)  # noqa: E731
    raw = torch.zeros(8192, dtype=torch.uint8, device=device)
    mark = lambda *shape: torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=device)  # noqa: E731
    # one column of size 5, blowup 1, log_last 1: two inner layers (sizes 4 and 3), 4 queries; h 2 keeps layers 1 .. 3, 1 .. 2, 1
    words, trees = rsv.fri_cap_sizes([5], 1, 1, 2)
    assert (words, trees) == (8 * (14 + 6 + 2), [0, 8 * 14, 8 * 20])
    a0 = {"quot": z(1, 128), "layers": z(1, 96), "sizes": [5], "b": 1, "last": 1, "q": z(1, 4), "nq": 4, "fw": mark(1, 3, 4, 4), "nf": mark(1, 3),
          "hw": mark(1, 3, 20, 8), "nh": mark(1, 3), "h": 2, "caps": z(words)}

    def refused(code, **kw):
        a = dict(a0, **kw)
        with pytest.raises(rsv.RsvError) as e:
            ctx.fri_open(a["quot"], a["layers"], a["sizes"], a["b"], a["last"], 1, a["q"], a["nq"], a["fw"], a["nf"], a["hw"], a["nh"],
                         sub_log=a["h"], d_caps=a["caps"])
        assert e.value.code == code, (code, e.value.code, kw)

    for k in ("quot", "layers", "q", "fw", "nf", "hw", "nh", "caps"):
        refused(-1, **{k: None})
    refused(-1, caps=None, nq=0)      # any NULL comes before any size
    refused(-1, quot=None, h=0)
    refused(-1, layers=None, h=9)
    refused(-2, sizes=[5, 5])
    refused(-2, sizes=[31])
    refused(-2, sizes=[5, 2])
    refused(-2, last=4)
    refused(-2, b=0)
    refused(-2, nq=0)
    refused(-2, nq=129)
    refused(-2, h=0)
    refused(-2, h=9)
    refused(-2, caps=raw[2:2 + 4 * words])
    refused(-2, q=raw[1:17])
    refused(-2, quot=raw[2:514])
    refused(-2, hw=raw[3:1923])
    ctx.synchronize()
    for k in ("fw", "nf", "hw", "nh"):
        assert bool((a0[k] == 0x5A5A5A5A).all()), k

    c0 = {"quot": z(1, 128), "sizes": [5], "b": 1, "last": 1, "chan": mark(1, 16), "roots": mark(1, 3, 8), "alphas": mark(1, 3, 4),
          "layers": mark(1, 96), "poly": mark(1, 2, 4), "low": torch.full((1,), 7, dtype=torch.uint8, device=device), "h": 2, "caps": mark(words)}

    def commit_refused(code, **kw):
        a = dict(c0, **kw)
        with pytest.raises(rsv.RsvError) as e:
            ctx.fri_commit(a["quot"], a["sizes"], a["b"], a["last"], 1, a["chan"], a["roots"], a["alphas"], a["layers"], a["poly"], a["low"],
                           sub_log=a["h"], d_caps=a["caps"])
        assert e.value.code == code, (code, e.value.code, kw)

    for k in ("quot", "chan", "roots", "alphas", "layers", "poly", "low"):
        commit_refused(-1, **{k: None})
    commit_refused(-1, roots=None, h=0)
    commit_refused(-2, sizes=[5, 6])
    commit_refused(-2, last=4)
    commit_refused(-2, h=0)
    commit_refused(-2, h=9)
    commit_refused(-2, caps=raw[1:1 + 4 * words])
    commit_refused(-2, chan=raw[2:66])
    ctx.synchronize()
    for k in ("chan", "roots", "alphas", "layers", "poly", "caps"):
        assert bool((c0[k] == 0x5A5A5A5A).all()), k
    assert int(c0["low"][0]) == 7
    ctx.close()


# ---------------------------------------------------------------- the fixture pairs
def _capped_chain(rsv, ctx, wp, pin):
    src, cfg = pin["src"], fixture_cfg(pin["dst"])
    ch = rsv.Chain(ctx, wp, 1, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, fri_sub_log=8, device=DEV)
    ch.witness([read_proof(src)], inputs_of(src))
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch, stage)()
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.open()
    ch.fri_open()
    return ch


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_capped_chain_outputs_the_next_fixture(rsv, pin):
    """Chain(caps=True, fri_sub_log=8) of fixture K through pow, open, fri_open and proofs(): fixture K+1's file byte for byte,
    and its layers' lists equal the stored ones in count and word for word, zero past the counts."""
    dst = pin["dst"]
    wp = program_of(rsv, pin)
    ctx = rsv.Context(0)
    ch = _capped_chain(rsv, ctx, wp, pin)
    assert ch.fri_caps is not None
    got, proofs = ch.numpy(), ch.proofs()
    ctx.close()
    wp.close()
    want = ob.split_variable_part(read_proof(dst))["layers"]
    assert got["ok"].tolist() == [1] and not (got["fri_caps"] == FILL).any()
    assert got["n_fri_witness"].shape == (1, len(want)) and got["n_fri_hash_witness"].shape == (1, len(want))
    for t, layer in enumerate(want):
        nf, nh = int(got["n_fri_witness"][0, t]), int(got["n_fri_hash_witness"][0, t])
        print(f"{pin['src']} -> {dst} layer {t}: fri_witness {nf} (stored {len(layer['fri_witness'])}), hash_witness {nh} (stored {len(layer['hash_witness'])})")
        assert (nf, nh) == (len(layer["fri_witness"]), len(layer["hash_witness"])), t
        assert np.array_equal(got["fri_witness"][0, t, :nf], np.array(layer["fri_witness"], np.uint32).reshape(-1, 4)), t
        assert np.array_equal(got["fri_hash_witness"][0, t, :nh], np.array(layer["hash_witness"], np.uint32).reshape(-1, 8)), t
        assert not got["fri_witness"][0, t, nf:].any() and not got["fri_hash_witness"][0, t, nh:].any(), t
        assert np.array_equal(got["fri_roots"][0, t], layer["commitment"]), t
    assert proofs[0] is not None and proofs[0] == read_proof(dst)


def test_capped_chain_packs_a_proof_the_verifier_accepts(rsv):
    """One pair through Chain.pack() into rsv_verify_batch_dev; caps=False on the same chain recomputes the same lists."""
    import torch
    pin = pin_of("level1-5.bin")
    dst = pin["dst"]
    wp = program_of(rsv, pin)
    ctx = rsv.Context(0)
    ch = _capped_chain(rsv, ctx, wp, pin)
    d_blob, d_offsets = ch.pack()
    acc = torch.full((1,), 7, dtype=torch.uint8, device=DEV)
    reason = torch.full((1,), 77, dtype=torch.uint8, device=DEV)
    ctx.verify_batch(d_blob, d_offsets, 1, acc, reason, cfg=fixture_cfg(dst), inputs=inputs_of(dst))
    ctx.synchronize()
    assert (acc.cpu().tolist(), reason.cpu().tolist()) == ([1], [0])
    capped = ch.numpy()
    ch.fri_open(caps=False)
    again = ch.numpy()
    for k in ("fri_witness", "n_fri_witness", "fri_hash_witness", "n_fri_hash_witness"):
        assert np.array_equal(capped[k], again[k]), k
    ctx.close()
    wp.close()
