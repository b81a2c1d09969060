"""rsv_fri_open_dev / Chain.fri_open (`-m gpu`): the openings of the FRI layer trees of the next proof.  On random quotient
columns through rsv_fri_commit_dev, bit for bit against the numpy restatement (tests/fri_open_ref.py, pinned to the stored
counts of every fixture by tests/test_fri_open_host.py) at the smallest shapes where a path changes, with the consumer's
walk of the device's lists back to the device's own roots; a masked proof, a workspace budget that cuts the proofs, the
refusals; and against the REFERENCE for all 14 consecutive fixture pairs: the chain of fixture K gives K+1's fri_witness and
hash_witness of every layer.  Every comparison is exact on 32-bit words; outputs are prefilled with 0xffffffff."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import fri_open_ref as FO
from tests import fri_ref as F
from tests import oracle_binding as ob
from tests.chain_harness import DEV, chain, dev, full, inputs_of, mask_dev, masked_past_64, pin_id, pins, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = C.P


def _commit_and_open(rsv, ctx, sizes, log_last, b, cols, queries, mask=None):
    """cols: per proof {size: (4, 2^size)}; queries [n][nq] -> dict of numpy outputs of fri_commit (roots, layers) and
    fri_open (fw [n, T, vcap, 4], nf [n, T], hw [n, T, wcap, 8], nh [n, T])."""
    import torch
    n, nq = len(cols), len(queries[0])
    ni = F.n_inner_of(sizes[0], log_last, b)
    T = 1 + ni
    lw = sum(4 << (sizes[0] - 1 - i) for i in range(ni))
    quot = np.stack([np.concatenate([c[s].reshape(-1) for s in sizes]) for c in cols])
    chan = dev(np.zeros((n, 16), np.uint32))
    roots, alphas, layers, last = full((n, T, 8)), full((n, T, 4)), full((n, max(lw, 1))), full((n, 1 << log_last, 4))
    low = torch.full((n,), 7, dtype=torch.uint8, device=torch.device(DEV))
    d_mask, d_quot, d_queries = mask_dev(mask), dev(quot), dev(np.asarray(queries, dtype=np.int64))
    ctx.fri_commit(d_quot, sizes, b, log_last, n, chan, roots, alphas, layers if ni else None, last, low, d_mask=d_mask)
    vcap, wcap = rsv.fri_open_sizes(sizes, b, log_last, nq)
    assert (vcap, wcap) == (len(sizes) * nq, nq * (sizes[0] + 2 * (len(sizes) - 1)))
    out = {"fw": full((n, T, vcap, 4)), "nf": full((n, T)), "hw": full((n, T, wcap, 8)), "nh": full((n, T))}
    ctx.fri_open(d_quot, layers if ni else None, sizes, b, log_last, n, d_queries, nq, out["fw"], out["nf"], out["hw"], out["nh"], d_mask=d_mask)
    ctx.synchronize()
    got = {k: u32(v) for k, v in out.items()}
    got["roots"], got["layers"] = u32(roots), u32(layers)
    return got


def _check_proof(got, p, sizes, log_last, b, cols, queries):
    """Proof p of a run against the restatement on the restated commitment, tree by tree; the walk of the device's lists."""
    M = sizes[0]
    want = F.commit(cols, log_last, b, C.Channel(ob, np.zeros(8, np.uint32), 0), ob)
    opened = FO.open_all(cols, want["layers"], queries, ob)
    assert got["nf"].shape[1] == len(opened)
    for t, ((top, layers), (fw, hw, root)) in enumerate(zip(FO.trees(cols, want["layers"]), opened)):
        nf, nh = int(got["nf"][p, t]), int(got["nh"][p, t])
        print(f"proof {p} tree {t}: fri_witness {nf} (want {len(fw)}), hash_witness {nh} (want {len(hw)})")
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


# (sizes, log_last, b): the smallest at which each path can go wrong
SHAPES = {
    "three_columns": ([7, 6, 5], 2, 1),
    "data_layer_under_the_top": ([6, 5], 1, 2),
    "joins_at_the_last_fold": ([6, 4], 1, 2),
    "no_inner_layer": ([4], 2, 1),
    "levels_past_one_workgroup": ([11, 9], 1, 1),
}
CASES = [(s, k) for s in SHAPES for k in ("one_query", "sixteen")] + [("no_inner_layer", "every_position"), ("width_256", "distinct_128")]


@pytest.mark.parametrize("shape,kind", CASES, ids=[f"{s}-{k}" for s, k in CASES])
def test_open_bit_for_bit(rsv, shape, kind):
    """Random quotient columns: counts and words of both lists of every tree equal the restatement's, zero past the counts,
    and the walk of the device's lists gives the device's own roots."""
    sizes, log_last, b = SHAPES.get(shape, ([9, 8, 6], 1, 1))
    rng = np.random.default_rng(2200 + CASES.index((shape, kind)))
    M = sizes[0]
    cols = {s: rng.integers(0, P, (4, 1 << s)) for s in sizes}
    if kind == "one_query":
        queries = [int(rng.integers(0, 1 << M)) | 1 << 31]  # bits above M are ignored
    elif kind == "sixteen":
        queries = _sixteen(rng, M)
    elif kind == "every_position":
        queries = rng.permutation(1 << M).tolist()
    else:
        queries = rng.choice(1 << M, 128, replace=False).tolist()
    ctx = rsv.Context(0)
    got = _commit_and_open(rsv, ctx, sizes, log_last, b, [cols], [queries])
    ctx.close()
    _check_proof(got, 0, sizes, log_last, b, cols, queries)
    if kind == "every_position":
        assert not got["nf"].any() and not got["nh"].any()


def test_batch_with_a_masked_proof(rsv):
    """Three proofs with their own columns and queries, the middle one masked: zero counts and zero buffers for it."""
    sizes, log_last, b = SHAPES["three_columns"]
    rng = np.random.default_rng(2230)
    cols = [{s: rng.integers(0, P, (4, 1 << s)) for s in sizes} for _ in range(3)]
    queries = [_sixteen(rng, sizes[0]) for _ in range(3)]
    ctx = rsv.Context(0)
    got = _commit_and_open(rsv, ctx, sizes, log_last, b, cols, queries, mask=[1, 0, 1])
    ctx.close()
    for k in ("fw", "nf", "hw", "nh"):
        assert not got[k][1].any(), k
    for p in (0, 2):
        _check_proof(got, p, sizes, log_last, b, cols[p], queries[p])


def test_past_one_workgroup_of_proofs(rsv):
    """70 proofs of the no_inner_layer shape with their own columns and four queries each, 63 and 64 masked: the second
    workgroup of the planner's per-proof rows, every live proof against the restatement."""
    sizes, log_last, b = SHAPES["no_inner_layer"]
    n, mask = 70, masked_past_64()
    rng = np.random.default_rng(2250)
    cols = [{s: rng.integers(0, P, (4, 1 << s)) for s in sizes} for _ in range(n)]
    queries = [rng.integers(0, 1 << sizes[0], 4).tolist() for _ in range(n)]
    ctx = rsv.Context(0)
    got = _commit_and_open(rsv, ctx, sizes, log_last, b, cols, queries, mask=mask)
    ctx.close()
    for p in range(n):
        if not mask[p]:
            assert all(not got[k][p].any() for k in ("fw", "nf", "hw", "nh")), p
        else:
            _check_proof(got, p, sizes, log_last, b, cols[p], queries[p])


def test_under_a_small_workspace_budget(rsv):
    """Five proofs of 2^13 leaves under a 1 MB budget.  The two node layers of a pass are 48 x 2^M bytes a proof (eight words
    a node, 2^M + 2^(M-1) nodes), whatever else the workspace holds: those of three proofs alone exceed the budget, so no pass
    holds more than two and the five proofs take at least three passes; those of two proofs leave a quarter of the budget
    for the plan (a few KB at 4 queries), so the driver's halving 5 -> 3 -> 2 stops at two.  Every word of the cut run equals
    the uncut run's, and one proof of the last pass the restatement's."""
    sizes, log_last, b, n, nq = [13, 11], 9, 1, 5, 4
    budget, node_bytes = 1 << 20, 48 << sizes[0]
    assert 3 * node_bytes > budget >= 2 * node_bytes + budget // 4
    rng = np.random.default_rng(2240)
    cols = [{s: rng.integers(0, P, (4, 1 << s)) for s in sizes} for _ in range(n)]
    queries = [rng.integers(0, 1 << sizes[0], nq).tolist() for _ in range(n)]
    ctx = rsv.Context(0)
    whole = _commit_and_open(rsv, ctx, sizes, log_last, b, cols, queries)
    ctx.set_option("ws_budget_mb", 1)
    cut = _commit_and_open(rsv, ctx, sizes, log_last, b, cols, queries)
    ctx.close()
    for k in whole:
        assert np.array_equal(cut[k], whole[k]), k
    _check_proof(whole, 4, sizes, log_last, b, cols[4], queries[4])


def test_device_refusals(rsv):
    """NULL pointers, sizes and misalignment with a live context: the neighbours' codes, nothing written."""
    import torch
    device = torch.device(DEV)
    ctx = rsv.Context(0)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)  # noqa: E731
    raw = torch.zeros(8192, dtype=torch.uint8, device=device)
    mark = lambda *shape: torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=device)  # noqa: E731
    # one column of size 5, blowup 1, log_last 1: two inner layers (sizes 4 and 3), 4 queries
    a0 = {"quot": z(1, 128), "layers": z(1, 96), "sizes": [5], "b": 1, "last": 1, "q": z(1, 4), "nq": 4, "fw": mark(1, 3, 4, 4), "nf": mark(1, 3),
          "hw": mark(1, 3, 20, 8), "nh": mark(1, 3)}
    assert rsv.fri_open_sizes([5], 1, 1, 4) == (4, 20)

    def refused(code, **kw):
        a = dict(a0, **kw)
        with pytest.raises(rsv.RsvError) as e:
            ctx.fri_open(a["quot"], a["layers"], a["sizes"], a["b"], a["last"], 1, a["q"], a["nq"], a["fw"], a["nf"], a["hw"], a["nh"])
        assert e.value.code == code, (code, e.value.code, kw)

    for k in ("quot", "layers", "q", "fw", "nf", "hw", "nh"):
        refused(-1, **{k: None})
    refused(-1, quot=None, nq=0)      # any NULL comes before any size
    refused(-1, layers=None, nq=129)
    refused(-2, sizes=[5, 5])
    refused(-2, sizes=[5, 6])
    refused(-2, sizes=[31])
    refused(-2, sizes=[5, 2])         # a column of log size 1 <= log_last
    refused(-2, last=4)
    refused(-2, sizes=[30], last=17)
    refused(-2, b=0)
    refused(-2, nq=0)
    refused(-2, nq=129)
    refused(-2, q=raw[1:17])
    refused(-2, quot=raw[2:514])
    refused(-2, fw=raw[1:193])
    refused(-2, hw=raw[3:1923])
    refused(-2, nh=raw[2:14])
    ctx.synchronize()
    for k in ("fw", "nf", "hw", "nh"):
        assert bool((a0[k] == 0x5A5A5A5A).all()), k
    ctx.close()


# ---------------------------------------------------------------- the fixture pairs
@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_chain_gives_the_next_fixtures_fri_openings(rsv, pin):
    """Chain.fri_open of fixture K: K+1's fri_witness and hash_witness of the first layer and of every inner layer, in count
    and word for word, zero past the counts."""
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    cfg = fixture_cfg(dst)
    ctx = rsv.Context(0)
    ch = chain(rsv, ctx, wp, [read_proof(src)], inputs_of(src), cfg.log_blowup_factor, upto="fri", log_last=cfg.log_last_layer_degree_bound)
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.fri_open()
    got = ch.numpy()
    ctx.close()
    wp.close()
    want = ob.split_variable_part(read_proof(dst))["layers"]
    assert got["ok"].tolist() == [1]
    assert got["n_fri_witness"].shape == (1, len(want)) and got["n_fri_hash_witness"].shape == (1, len(want))
    for t, layer in enumerate(want):
        nf, nh = int(got["n_fri_witness"][0, t]), int(got["n_fri_hash_witness"][0, t])
        print(f"{src} -> {dst} layer {t}: fri_witness {nf} (stored {len(layer['fri_witness'])}), hash_witness {nh} (stored {len(layer['hash_witness'])})")
        assert (nf, nh) == (len(layer["fri_witness"]), len(layer["hash_witness"])), t
        assert np.array_equal(got["fri_witness"][0, t, :nf], np.array(layer["fri_witness"], np.uint32).reshape(-1, 4)), t
        assert np.array_equal(got["fri_hash_witness"][0, t, :nh], np.array(layer["hash_witness"], np.uint32).reshape(-1, 8)), t
        assert not got["fri_witness"][0, t, nf:].any() and not got["fri_hash_witness"][0, t, nh:].any(), t
        assert np.array_equal(got["fri_roots"][0, t], layer["commitment"]), t
