"""The caps of the FRI layer trees, host side, without a device: the four entry points exist, rsv_fri_cap_sizes and its
refusals, every refusal of rsv_fri_commit_cap_dev, rsv_witness_fri_caps_dev and rsv_fri_open_cap_dev returns before any device
work, and the rule the capped opening lists its subtrees by, pinned on tests/fri_open_ref.py: the layer-c ancestors of the
planned witness nodes above layer c lie in S_c and number at most twice the queries."""
import ctypes

import numpy as np
import pytest

from tests import fri_open_ref as FO

NEW = ("rsv_fri_cap_sizes", "rsv_fri_commit_cap_dev", "rsv_witness_fri_caps_dev", "rsv_fri_open_cap_dev")


def kept(top, h):
    """c: a tree with leaves at `top` keeps its layers 1 .. c."""
    return max(top - h, 0)


def test_entry_points_exist(rsv):
    for name in NEW:
        assert name in rsv.EXPORTS and hasattr(rsv.lib, name), name
    assert callable(rsv.fri_cap_sizes)
    assert rsv.lib.rsv_abi_version() == 6


def test_fri_cap_sizes(rsv):
    """Per proof the sum over the trees of 8 (2^(c_t + 1) - 2) words; the trees one after another; n proofs n times that."""
    sizes, b, last, h = [18, 17, 16], 1, 0, 8
    tops = [18 - t for t in range(17)]  # the first layer and 16 inner layers
    per_tree = [8 * ((2 << kept(top, h)) - 2) for top in tops]
    words, trees = rsv.fri_cap_sizes(sizes, b, last, h)
    assert words == sum(per_tree) and trees == np.cumsum([0] + per_tree[:-1]).tolist()
    assert per_tree[0] == 8 * 2046 and per_tree[9] == 8 * 2 and not any(per_tree[10:])
    words16, trees16 = rsv.fri_cap_sizes(sizes, b, last, h, 16)
    assert words16 == 16 * words and trees16 == [16 * w for w in trees]
    assert rsv.fri_cap_sizes([4], 1, 2, 4) == (0, [0])            # top == h: nothing is kept
    assert rsv.fri_cap_sizes([7, 6, 5], 1, 2, 1, 3) == (3 * 8 * (126 + 62 + 30 + 14), [0, 3 * 8 * 126, 3 * 8 * 188, 3 * 8 * 218])


def test_fri_cap_sizes_refusals(rsv):
    lib = rsv.lib
    sz = np.array([7, 6, 5], np.uint32)
    p, words = sz.ctypes.data_as(rsv._u32p), ctypes.c_size_t()
    assert lib.rsv_fri_cap_sizes(None, 3, 1, 2, 3, 1, ctypes.byref(words), None) == -1
    assert lib.rsv_fri_cap_sizes(p, 3, 1, 2, 3, 1, None, None) == -1
    assert lib.rsv_fri_cap_sizes(p, 3, 1, 2, 3, 1, ctypes.byref(words), None) == 0
    for bad in (([], 1, 1, 3, 1), ([4, 4], 1, 1, 3, 1), ([4, 5], 1, 1, 3, 1), ([31], 1, 1, 3, 1), ([4, 2], 1, 1, 3, 1), ([4], 1, 3, 3, 1),
                ([4], 0, 1, 3, 1), ([30], 1, 17, 3, 1), ([9] * 9, 1, 1, 3, 1), ([7, 6, 5], 1, 2, 0, 1), ([7, 6, 5], 1, 2, 9, 1),
                ([7, 6, 5], 1, 2, 3, (1 << 20) + 1)):
        with pytest.raises(rsv.RsvError) as e:
            rsv.fri_cap_sizes(*bad)
        assert e.value.code == -2, bad


def test_refusals_need_no_device(rsv):
    """Every refusal of the three _dev calls comes before any device work: a context that is 64 zero bytes and device
    pointers that are plain numbers are never dereferenced.  Without a device what passes the refusals is RSV_E_DEVICE."""
    lib = rsv.lib
    ctx = ctypes.cast(ctypes.create_string_buffer(8192), ctypes.c_void_p)
    prog = ctypes.cast(ctypes.create_string_buffer(8192), ctypes.c_void_p)
    buf, odd = ctypes.c_void_p(8192), ctypes.c_void_p(8194)

    def sizes_p(sizes):
        a = np.array(sizes, np.uint32)
        return a, a.ctypes.data_as(rsv._u32p)

    def commit(ctx=ctx, quot=buf, sizes=(5,), b=1, last=1, n=1, chan=buf, roots=buf, alphas=buf, layers=buf, poly=buf, low=buf, h=3, caps=buf):
        keep, p = sizes_p(sizes)
        return lib.rsv_fri_commit_cap_dev(ctx, quot, p if sizes is not None else None, len(keep), b, last, n, None, chan, roots, alphas, layers, poly,
                                          low, h, caps)

    for k in ("ctx", "quot", "chan", "roots", "alphas", "layers", "poly", "low"):
        assert commit(**{k: None}) == -1, k
    assert commit(quot=None, h=0) == -1 and commit(roots=None, caps=odd) == -1  # any NULL comes before any size
    for kw in ({"sizes": (5, 5)}, {"sizes": (5, 6)}, {"sizes": (31,)}, {"sizes": (5, 2)}, {"last": 4}, {"b": 0}, {"n": (1 << 20) + 1},
               {"h": 0}, {"h": 9}, {"caps": odd}, {"quot": odd}, {"layers": odd}, {"poly": odd}):
        assert commit(**kw) == -2, kw
    assert commit(n=0) == 0 and commit(n=0, caps=None) == 0  # an empty batch is no work
    # d_caps NULL: rsv_fri_commit_dev, which reads no sub_log
    assert commit(caps=None, h=0, quot=None) == -1 and commit(caps=None, h=77, sizes=(5, 5)) == -2

    def opening(ctx=ctx, quot=buf, layers=buf, sizes=(5,), b=1, last=1, n=1, q=buf, nq=4, fw=buf, nf=buf, hw=buf, nh=buf, h=3, caps=buf):
        keep, p = sizes_p(sizes)
        return lib.rsv_fri_open_cap_dev(ctx, quot, layers, p, len(keep), b, last, n, None, q, nq, fw, nf, hw, nh, h, caps)

    for k in ("ctx", "quot", "layers", "q", "fw", "nf", "hw", "nh", "caps"):
        assert opening(**{k: None}) == -1, k
    assert opening(caps=None, nq=0) == -1 and opening(caps=None, h=0) == -1 and opening(layers=None, nq=129) == -1
    for kw in ({"sizes": (5, 5)}, {"sizes": (31,)}, {"sizes": (5, 2)}, {"last": 4}, {"b": 0}, {"nq": 0}, {"nq": 129}, {"h": 0}, {"h": 9},
               {"caps": odd}, {"q": odd}, {"quot": odd}, {"fw": odd}, {"hw": odd}, {"nh": odd}, {"n": (1 << 20) + 1}):
        assert opening(**kw) == -2, kw
    assert opening(n=0) == 0

    def chain(ctx=ctx, prog=prog, plonk=buf, comp=buf, chan=buf, quot=buf, roots=buf, layers=buf, h=3, caps=buf, n=1):
        return lib.rsv_witness_fri_caps_dev(ctx, prog, plonk, buf, buf, buf, buf, buf, None, n, 1, 0, comp, buf, buf, buf, chan, buf, quot, roots, buf,
                                            layers, buf, buf, h, caps)

    for k in ("ctx", "prog", "plonk", "comp", "chan", "quot", "roots"):
        assert chain(**{k: None}) == -1, k
    assert chain(plonk=None, h=0) == -1 and chain(plonk=None, caps=odd) == -1
    for kw in ({"h": 0}, {"h": 9}, {"caps": odd}, {"quot": odd}, {"layers": odd}, {"n": (1 << 20) + 1}):
        assert chain(**kw) == -2, kw
    assert chain() == -2 and chain(caps=None) == -2  # a program that was not built (no gates): after every pointer's check
    if rsv.device_count() == 0:
        assert commit() == -3 and commit(caps=None) == -3 and commit(sizes=(7, 6, 5), last=2, h=8) == -3
        assert opening() == -3 and opening(sizes=(7, 6, 5), last=2, h=1, nq=128) == -3


# ---------------------------------------------------------------- the subtree rule
def ancestors(top, D, h, queries):
    """The subtrees a capped opening rebuilds: the layer-c ancestors of plan()'s witness nodes above layer c."""
    c = kept(top, h)
    return c, sorted({x >> (l - c) for l, x in FO.plan(top, D, queries)[1] if l > c})


def test_subtrees_lie_in_S_c_and_are_at_most_two_per_query():
    """3 000 random (top, data layers, h, queries): the ancestors are inside S_c, inside Q_c unless c is a data layer, at most
    2 n_queries, and every planned node at a layer <= c is a kept one (1 <= l)."""
    rng = np.random.default_rng(2600)
    past_Q = 0
    for _ in range(3000):
        top = int(rng.integers(2, 14))
        D = {top} | {int(x) for x in rng.integers(2, top + 1, int(rng.integers(0, 3)))}
        h = int(rng.integers(1, 9))
        nq = int(rng.integers(1, 20))
        queries = rng.integers(0, 1 << top, nq).tolist()
        c, subs = ancestors(top, D, h, queries)
        Q, S = FO.sets(top, D, queries)
        assert set(subs) <= set(S[c]), (top, D, h, queries)
        assert len(subs) <= 2 * nq
        if c not in D:
            assert set(subs) <= set(Q[c]), (top, D, h, queries)
        elif not set(subs) <= set(Q[c]):
            past_Q += 1
        assert all(l >= 1 for l, _ in FO.plan(top, D, queries)[1])
    assert past_Q  # the case below is met at random as well


def test_a_sibling_nobody_queries_brings_its_own_subtree():
    """top 7, data layers {7, 4}, h 3, query 0: c = 4 is a data layer; node 1 of layer 4 is a sibling nobody queries, both its
    children (layer 5, positions 2 and 3) are witnesses, and they lie in subtree 1, which no query touches."""
    fri, hw = FO.plan(7, {7, 4}, [0])
    assert (4, 1) in fri and (5, 2) in hw and (5, 3) in hw
    assert ancestors(7, {7, 4}, 3, [0]) == (4, [0, 1])
    assert ancestors(7, {7}, 3, [0]) == (4, [0])
    # h = 1: a queried pair needs nothing from its own two-leaf subtree; only the sibling's subtree is rebuilt
    assert ancestors(7, {7, 6}, 1, [0]) == (6, [1])
    assert ancestors(4, {4}, 4, [3]) == (0, [0]) and ancestors(4, {4}, 8, range(16)) == (0, [])
