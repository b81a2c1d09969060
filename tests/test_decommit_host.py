"""Decommitment of trees 0, 1 and 2 of the next proof (no device).  The numpy restatement in tests/decommit_ref.py is pinned
in both directions: (a) on the cheapest fixture pair, recursive_proof_16_15 x5 -> level1-5, with the columns of the
oracle's circuit, its output at level1-5's query positions is level1-5's queried_values[t] and hash_witness[t], counts
included; (b) on random mixed-size trees the verifier's walk fed with its output reproduces commit_ref.merkle_root.
tests/test_decommit_gpu.py compares the device against this helper.  Also: rsv_decommit_sizes and the argument refusals of
the new entry points, which need no device."""
import ctypes

import numpy as np
import pytest

from tests import commit_ref as C
from tests import decommit_ref as D
from tests import interaction_ref as R
from tests import oracle_binding as ob
from tests.conftest import fixture_cfg, read_proof
from tests.chain_harness import oracle_columns

P = C.P


def test_restatement_reproduces_the_next_fixture_decommitment():
    ppre, ptr, qpre, qtr, lp, lq, dst = oracle_columns("recursive_proof_16_15.bin")
    nxt = read_proof(dst)
    b = fixture_cfg(dst).log_blowup_factor
    tr = ob.transcript_raw(nxt)
    z, alpha = tuple(int(x) for x in tr[4:8]), tuple(int(x) for x in tr[8:12])
    want = ob.split_variable_part(nxt)
    qM, M = C.query_positions(nxt, ob)
    for t in range(3):
        if t == 0:
            groups = [(lp, ppre), (lq, qpre)]
        elif t == 1:
            groups = [(lp, ptr), (lq, qtr)]
        else:
            cp, cq, _, ok = R.interaction(ppre, ptr, qpre, qtr, z, alpha, lp, lq)
            assert ok
            groups = [(lp, cp), (lq, cq)]
        layers = C.tree_layers(groups, b)
        top = max(layers)
        values, witness, _ = D.decommit(layers, qM >> (M - top), ob)
        wv, ww = want["queried_values"][t], want["hash_witness"][t]
        print(f"tree {t}: {len(values)} values (fixture {len(wv)}), {len(witness)} witness nodes (fixture {len(ww)})")
        assert len(values) == len(wv) and values.tolist() == [int(x) for x in wv], t
        assert len(witness) == len(ww) and np.array_equal(witness, np.array(ww, np.uint32).reshape(-1, 8)), t
        del layers


def _random_tree(rng, spec, b):
    groups = [(log, rng.integers(0, P, (nc, 1 << log))) for log, nc in spec]
    layers = C.tree_layers(groups, b)
    ncols_at = {l: len(c) for l, c in layers.items()}
    return layers, ncols_at


QUERY_CASES = ["one", "dup", "128", "one_block", "sibling_pairs", "all_leaves"]


def _queries(kind, rng, top, b):
    if kind == "one":
        return rng.integers(0, 1 << top, 1)
    if kind == "dup":
        q = rng.integers(0, 1 << top, 5)
        return np.concatenate([q, q[:3], q[1:2]])
    if kind == "128":
        return rng.integers(0, 1 << 32, 128)  # bits above top are ignored
    if kind == "one_block":
        blk = int(rng.integers(0, 1 << b))
        return (blk << (top - b)) + rng.integers(0, 1 << (top - b), 9)
    if kind == "sibling_pairs":
        q = rng.integers(0, 1 << top, 6)
        return np.concatenate([q, q[:4] ^ 1, (q[4:] ^ 2)])  # four leaf sibling pairs (no witness at the leaves), two cousin pairs (none one layer down)
    return np.arange(min(1 << top, 128))


@pytest.mark.parametrize("kind", QUERY_CASES)
@pytest.mark.parametrize("case", range(4))
def test_walk_of_the_restatement_gives_the_root(case, kind):
    spec, b = [([(5, 3)], 1), ([(4, 2), (6, 9)], 3), ([(0, 1), (1, 2), (2, 3), (3, 17)], 5), ([(5, 4), (5, 12), (3, 1)], 4)][case]
    rng = np.random.default_rng(1000 + 10 * case + QUERY_CASES.index(kind))
    layers, ncols_at = _random_tree(rng, spec, b)
    top = max(layers)
    q = _queries(kind, rng, top, b)
    values, witness, cap = D.decommit(layers, q, ob, b)
    root = C.merkle_root(layers, ob)
    assert D.walk(values, witness, q, ncols_at, top, ob).tolist() == root.tolist()
    assert cap[1].tolist() == root.tolist() and not cap[0].any()
    nodes, wit = D.plan(q, top)
    assert len(values) == sum(len(nodes[l]) * ncols_at.get(l, 0) for l in nodes)
    assert len(witness) == sum(len(w) for w in wit.values())
    if kind == "sibling_pairs":
        assert len(wit[top]) <= 4  # the four queried pairs need none: at most the two cousin pairs' leaf siblings
    if kind == "all_leaves" and (1 << top) <= 128:
        assert len(witness) == 0
    # a leftover or a missing word is noticed
    with pytest.raises(AssertionError):
        D.walk(np.concatenate([values, values[:1]]), witness, q, ncols_at, top, ob)
    if len(witness):
        with pytest.raises(AssertionError):
            D.walk(values, witness[:-1], q, ncols_at, top, ob)
        bad = witness.copy()
        bad[0, 0] ^= 1
        assert D.walk(values, bad, q, ncols_at, top, ob).tolist() != root.tolist()


def test_sizes_and_argument_validation_need_no_device(rsv):
    """rsv_decommit_sizes is host arithmetic; every refusal of the device entry points returns before any device work."""
    lib = rsv.lib
    assert all(k in rsv.EXPORTS for k in ("rsv_decommit_sizes", "rsv_decommit_tree_dev", "rsv_commit_tree_cap_dev", "rsv_witness_decommit_dev",
                                          "rsv_witness_commit_caps_dev"))
    assert rsv.decommit_sizes([(16, 12), (15, 48)], 8, 16) == (16 * 60, 16 * 24)
    assert rsv.decommit_sizes([(3, 1)], 1, 128) == (128, 128 * 4)
    for bad in (lambda: rsv.decommit_sizes([(3, 1)], 0, 16), lambda: rsv.decommit_sizes([(3, 1)], 2, 0), lambda: rsv.decommit_sizes([(3, 1)], 2, 129),
                lambda: rsv.decommit_sizes([(29, 1)], 2, 16), lambda: rsv.decommit_sizes([(3, 0)], 2, 16), lambda: rsv.decommit_sizes([(3, 1)] * 9, 2, 16)):
        with pytest.raises(rsv.RsvError) as e:
            bad()
        assert e.value.code == -2
    v, w = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.rsv_decommit_sizes(None, 1, 2, 16, ctypes.byref(v), ctypes.byref(w)) == -1
    fake = ctypes.create_string_buffer(64)  # never dereferenced: every refusal below comes first
    fake_p = ctypes.cast(fake, ctypes.c_void_p)
    buf = ctypes.c_void_p(8192)

    def groups(*specs):
        arr = (rsv.CommitGroup * len(specs))()
        for k, (log, nc, ptr) in enumerate(specs):
            arr[k] = rsv.CommitGroup(log, nc, ptr, nc << log, None, None)
        return arr

    g = groups((4, 2, ctypes.c_void_p(4096)))

    def call(ctx=fake_p, gr=g, ng=1, b=2, q=buf, nq=16, mode=0, cap=None, values=buf, nv=buf, wit=buf, nw=buf):
        return lib.rsv_decommit_tree_dev(ctx, gr, ng, 1, b, None, q, nq, mode, cap, values, nv, wit, nw)

    assert call(ctx=None) == -1 and call(gr=None) == -1 and call(q=None) == -1 and call(values=None) == -1 and call(nv=None) == -1
    assert call(wit=None) == -1 and call(nw=None) == -1
    assert call(gr=groups((4, 2, None))) == -1
    assert call(mode=rsv.CAP_READ) == -1 and call(mode=rsv.CAP_WRITE) == -1  # no buffer
    assert call(mode=3, cap=buf) == -2 and call(mode=-1) == -2
    assert call(nq=0) == -2 and call(nq=129) == -2
    assert call(b=0) == -2 and call(b=17) == -2
    assert call(ng=0) == -2 and call(gr=groups(*[(4, 2, ctypes.c_void_p(4096))] * 9), ng=9) == -2
    assert call(gr=groups((29, 2, ctypes.c_void_p(4096)))) == -2 and call(gr=groups((4, 0, ctypes.c_void_p(4096)))) == -2
    odd = ctypes.c_void_p(8194)
    assert call(q=odd) == -2 and call(values=odd) == -2 and call(wit=odd) == -2 and call(nv=odd) == -2 and call(nw=odd) == -2
    assert call(mode=rsv.CAP_READ, cap=odd) == -2 and call(gr=groups((4, 2, ctypes.c_void_p(4098)))) == -2
    assert lib.rsv_commit_tree_cap_dev(None, g, 1, 1, 2, None, buf, buf) == -1
    assert lib.rsv_commit_tree_cap_dev(fake_p, g, 1, 1, 2, None, buf, odd) == -2
    assert lib.rsv_commit_tree_cap_dev(fake_p, g, 1, 1, 0, None, buf, buf) == -2
    assert lib.rsv_witness_decommit_dev(*([None] * 9), 0, 2, None, 16, None, None, None, None, None) == -1
    args = [fake_p, fake_p] + [buf] * 7
    assert lib.rsv_witness_decommit_dev(*args, 1, 0, buf, 16, None, buf, buf, buf, buf) == -2
    assert lib.rsv_witness_decommit_dev(*args, 1, 2, buf, 0, None, buf, buf, buf, buf) == -2
    assert lib.rsv_witness_decommit_dev(*args, 1, 2, buf, 129, None, buf, buf, buf, buf) == -2
    assert lib.rsv_witness_decommit_dev(*args, 1, 2, odd, 16, None, buf, buf, buf, buf) == -2
    assert lib.rsv_witness_commit_caps_dev(*([None] * 6), 0, 2, *([None] * 8)) == -1
    assert lib.rsv_witness_commit_caps_dev(fake_p, fake_p, buf, buf, buf, buf, 1, 2, buf, buf, buf, buf, buf, None, None, odd) == -2
