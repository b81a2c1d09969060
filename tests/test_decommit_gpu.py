"""rsv_decommit_tree_dev / rsv_commit_tree_cap_dev / rsv_witness_decommit_dev / rsv_witness_commit_caps_dev (`-m gpu`): the
opening of trees 0, 1 and 2 of the next proof.  Against the REFERENCE for all 14 consecutive fixture pairs (the values and
witness nodes are K+1's queried_values[t] and hash_witness[t], word for word and in count, with nothing taken from K+1 but
log_blowup_factor, n_queries and the positions), bit for bit against the numpy restatement (tests/decommit_ref.py, pinned
to the fixtures by tests/test_decommit_host.py) on random trees in the three cap modes, the cap being trusted, and the
refusals."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import decommit_ref as D
from tests import oracle_binding as ob
from tests.chain_harness import CASES, DEV, chain, dev, full, inputs_of, mask_dev, masked_past_64, pin_id, pins, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = C.P


def _witness_decommit(rsv, ch, queries, caps):
    """Chain.decommit -> per proof and tree (values, witness) cut at the counts; the words past them are zero."""
    n = ch.n
    vcaps, wcap = rsv.witness_decommit_sizes(ch.program, ch.log_blowup, queries.shape[1])
    d_v, d_w, d_nv, d_nw = full((n, sum(vcaps))), full((n, 3, wcap, 8)), full((n, 3)), full((n, 3))
    d_q = dev(queries)
    ch.decommit(d_q, d_v, d_nv, d_w, d_nw, caps=caps)
    ch.ctx.synchronize()
    v, w, nv, nw = u32(d_v), u32(d_w), u32(d_nv), u32(d_nw)
    out = []
    for p in range(n):
        off, per = 0, []
        for k in range(3):
            vals, wit = v[p, off:off + vcaps[k]], w[p, k]
            assert nv[p, k] <= vcaps[k] and nw[p, k] <= wcap
            assert not vals[nv[p, k]:].any() and not wit[nw[p, k]:].any(), (p, k)
            per.append((vals[:nv[p, k]].copy(), wit[:nw[p, k]].copy()))
            off += vcaps[k]
        out.append(per)
    return out


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_chain_opens_what_the_next_fixture_decommits(rsv, pin):
    """The library alone, with K+1's log_blowup_factor, n_queries and query positions and nothing else from K+1: for t = 0,
    1, 2 the values and witness nodes are K+1's queried_values[t] and hash_witness[t], in count and word for word, and zero
    past the counts; the call without caps gives identical outputs."""
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    cfg = fixture_cfg(dst)
    b = cfg.log_blowup_factor
    nxt = read_proof(dst)
    qM, M = C.query_positions(nxt, ob)
    assert len(qM) == cfg.n_queries
    top = max(wp.trace_sizes()) + b
    q = (qM >> (M - top)).astype(np.uint32)[None]
    ctx = rsv.Context(0)
    ch = chain(rsv, ctx, wp, [read_proof(src)], inputs_of(src), b, caps=True)
    with_caps = _witness_decommit(rsv, ch, q, caps=True)[0]
    without = _witness_decommit(rsv, ch, q, caps=False)[0]
    ctx.close()
    want = ob.split_variable_part(nxt)
    for k in range(3):
        wv = np.array([int(x) for x in want["queried_values"][k]], np.uint32)
        ww = np.array(want["hash_witness"][k], np.uint32).reshape(-1, 8)
        for label, (vals, wit) in (("caps", with_caps[k]), ("no caps", without[k])):
            print(f"{src} tree {k} {label}: {len(vals)} values (fixture {len(wv)}), {len(wit)} witness nodes (fixture {len(ww)})")
            assert len(vals) == len(wv) and np.array_equal(vals, wv), (k, label)
            assert len(wit) == len(ww) and np.array_equal(wit, ww), (k, label)
    wp.close()


def test_chain_masked_proof_and_batch(rsv):
    """Five proofs, the third tampered (rejected), per-proof different queries: the rejected proof gets zero counts and zero
    buffers, the others what their solo run gives."""
    pin = next(p for p in pins() if p["src"] == "recursive_proof_16_15.bin")
    wp = program_of(rsv, pin)
    src = pin["src"]
    b = fixture_cfg(pin["dst"]).log_blowup_factor
    proof = read_proof(src)
    batch = [proof, proof, ob.tamper(proof, 5), proof, proof]
    top = max(wp.trace_sizes()) + b
    q = np.random.default_rng(5).integers(0, 1 << top, (5, 16)).astype(np.uint32)
    ctx = rsv.Context(0)
    ch = chain(rsv, ctx, wp, batch, inputs_of(src), b, caps=True)
    got = _witness_decommit(rsv, ch, q, caps=True)
    assert ch.ok.cpu().tolist() == [1, 1, 0, 1, 1]
    solo_ch = chain(rsv, ctx, wp, [proof], inputs_of(src), b, caps=True)
    for p in range(5):
        if p == 2:
            assert all(len(v) == 0 and len(w) == 0 for v, w in got[p])
            continue
        solo = _witness_decommit(rsv, solo_ch, q[p:p + 1], caps=(p & 1) == 0)[0]
        for k in range(3):
            assert np.array_equal(got[p][k][0], solo[k][0]) and np.array_equal(got[p][k][1], solo[k][1]), (p, k)
    ctx.close()
    wp.close()


def _groups_dev(groups, shared):
    gs = []
    for i, (log, cols) in enumerate(groups):
        nc = cols.shape[1]
        gs.append({"log_size": log, "d_cols": dev(np.asarray(cols, dtype=np.int64) % P), "n_cols": nc, "proof_stride": 0 if i in shared else nc << log})
    return gs


def _decommit_dev(rsv, ctx, gs, b, n, queries, mask=None, mode=0, cap=None):
    """Context.decommit_tree -> (values [n][vcap], n_values, witness [n][wcap][8], n_witness, cap tensor or None)."""
    nq = queries.shape[1]
    vcap, wcap = rsv.decommit_sizes(gs, b, nq)
    d_v, d_w, d_nv, d_nw = full((n, vcap)), full((n, wcap, 8)), full((n,)), full((n,))
    if mode == rsv.CAP_WRITE:
        cap = full((n, 2 << b, 8))
    d_q, d_mask = dev(queries), mask_dev(mask)
    ctx.decommit_tree(gs, n, b, d_q, nq, d_v, d_nv, d_w, d_nw, d_mask=d_mask, cap_mode=mode, d_cap=cap)
    ctx.synchronize()
    return u32(d_v), u32(d_nv), u32(d_w), u32(d_nw), cap


def _commit_cap(rsv, ctx, gs, b, n, mask, with_cap):
    d_roots = full((n, 8))
    d_cap = full((n, 2 << b, 8)) if with_cap else None
    d_mask = mask_dev(mask)
    ctx.commit_tree(gs, n, b, d_roots, d_mask, d_cap=d_cap)
    ctx.synchronize()
    return u32(d_roots), d_cap


def _queries(rng, n, nq, top, b, kind):
    q = rng.integers(0, 1 << 32, (n, nq)).astype(np.uint32)  # bits above top are ignored
    if kind == "dup" and nq >= 4:
        q[:, nq // 2:] = q[:, :nq - nq // 2]          # every position twice, unsorted
        q[:, 1] = q[:, 0] ^ 1                         # a sibling pair: no witness node at the leaves for it
    if kind == "one_block":
        q = ((q[:, :1] >> (32 - b)).astype(np.uint64) << (top - b) | (q & ((1 << (top - b)) - 1))).astype(np.uint32)
    return q


def _check_case(rsv, ctx, spec, b, n, mask, nq, seed, kind="dup", budget_cut=None):
    """One random tree: in the three cap modes the outputs equal the restatement's, element by element and in count, zero
    past the counts; CAP_WRITE's cap = the restatement's = commit_tree(d_cap=)'s; the roots do not depend on d_cap."""
    rng = np.random.default_rng(seed)
    groups = [(log, rng.integers(0, P, (1 if sh else n, nc, 1 << log))) for log, nc, sh in spec]
    shared = {i for i, (_, _, sh) in enumerate(spec) if sh}
    top = max(log for log, _, _ in spec) + b
    q = _queries(rng, n, nq, top, b, kind)
    gs = _groups_dev(groups, shared)
    none = _decommit_dev(rsv, ctx, gs, b, n, q, mask, rsv.CAP_NONE)
    write = _decommit_dev(rsv, ctx, gs, b, n, q, mask, rsv.CAP_WRITE)
    read = _decommit_dev(rsv, ctx, gs, b, n, q, mask, rsv.CAP_READ, cap=write[4])
    roots, _ = _commit_cap(rsv, ctx, gs, b, n, mask, False)
    roots_c, cap_c = _commit_cap(rsv, ctx, gs, b, n, mask, True)
    assert np.array_equal(roots, roots_c)
    cap_w, cap_c = u32(write[4]), u32(cap_c)
    assert np.array_equal(cap_w, cap_c)
    for label, other in (("write", write), ("read", read)):
        for k in range(4):
            assert np.array_equal(none[k], other[k]), (label, k)
    if budget_cut is not None:
        ctx.set_option("ws_budget_mb", budget_cut)
        for mode, cap in ((rsv.CAP_NONE, None), (rsv.CAP_READ, write[4])):
            cut = _decommit_dev(rsv, ctx, gs, b, n, q, mask, mode, cap=cap)
            for k in range(4):
                assert np.array_equal(none[k], cut[k]), ("cut", mode, k)
        ctx.set_option("ws_budget_mb", 8192)
    values, nv, wit, nw, _ = none
    for p in range(n):
        if mask is not None and not mask[p]:
            assert nv[p] == 0 and nw[p] == 0 and not values[p].any() and not wit[p].any() and not cap_w[p].any(), p
            continue
        mine = [(log, cols[0 if i in shared else p]) for i, (log, cols) in enumerate(groups)]
        layers = C.tree_layers(mine, b)
        rv, rw, rcap = D.decommit(layers, q[p], ob, b)
        assert nv[p] == len(rv) and nw[p] == len(rw), (p, nv[p], len(rv), nw[p], len(rw))
        assert np.array_equal(values[p, :nv[p]], rv) and not values[p, nv[p]:].any(), p
        assert np.array_equal(wit[p, :nw[p]], rw) and not wit[p, nw[p]:].any(), p
        assert np.array_equal(cap_w[p], rcap) and roots[p].tolist() == rcap[1].tolist(), p
    return groups, q, gs, write[4], none


@pytest.mark.parametrize("case", range(len(CASES)))
def test_decommit_tree_bit_for_bit(rsv, case):
    """The shapes of test_commit_gpu.CASES, 7 queries with duplicates and a sibling pair, per-proof different."""
    spec, b, n, mask = CASES[case]
    ctx = rsv.Context(0)
    _check_case(rsv, ctx, spec, b, n, mask, 7, 500 + case)
    ctx.close()


def test_decommit_tree_past_one_workgroup_of_proofs(rsv):
    """The first of CASES with 70 proofs, four queries that differ per proof, 63 and 64 masked: the second workgroup of the
    planner's per-proof rows, every proof against the restatement."""
    spec, b, _, _ = CASES[0]
    ctx = rsv.Context(0)
    _check_case(rsv, ctx, spec, b, 70, masked_past_64(), 4, 950, kind="any")
    ctx.close()


WIDE = [  # (groups, b, n, mask, nq, kind)
    ([(4, 3, False), (6, 2, False)], 8, 2, None, 1, "any"),
    ([(4, 3, False), (6, 2, False)], 8, 2, None, 16, "dup"),
    ([(4, 3, False), (6, 2, False)], 8, 1, None, 128, "any"),
    ([(5, 2, False)], 9, 1, None, 1, "any"),
    ([(5, 2, False), (3, 4, False)], 9, 2, None, 16, "one_block"),
    ([(3, 1, False)], 9, 1, None, 128, "dup"),
    ([(11, 2, False), (7, 3, False)], 3, 2, None, 16, "dup"),   # below CM_LDS_LOG = 12: the LDS pass alone
    ([(13, 1, False), (9, 2, True)], 3, 2, None, 16, "dup"),    # above: one global forward pass reading the coefficients
    ([(6, 5, True), (5, 7, False)], 4, 5, [1, 1, 0, 1, 1], 9, "dup"),
    ([(2, 3, False)], 2, 3, None, 128, "any"),                   # every leaf queried many times over: no witness at all
    ([(0, 2, False), (3, 1, False)], 2, 2, [0, 1], 5, "dup"),    # a log-0 group: its values sit at layer b, the block roots'
]


def test_decommit_tree_wide_blowups_passes_and_masks(rsv):
    """log_blowup 8 and 9 with 1, 16 and 128 queries (most blocks untouched), all queries in one block, logs 11 and 13 across
    the LDS / global-pass boundary mixed with a smaller group, n = 5 with a masked proof, a tiny tree with every leaf queried,
    a log-0 group."""
    ctx = rsv.Context(0)
    for case, (spec, b, n, mask, nq, kind) in enumerate(WIDE):
        _check_case(rsv, ctx, spec, b, n, mask, nq, 700 + case, kind)
    ctx.close()


def test_decommit_under_a_small_workspace_budget(rsv):
    """41 proofs at b = 4, a log-9 and a log-8 group, three masked, 7 queries: under a 1 MB budget the opening is cut into
    passes of fewer list entries and fewer proofs with a short last one, in CAP_NONE (16 blocks a proof) and in CAP_READ
    (at most 7); both equal the uncut run, and the uncut run the restatement."""
    mask = [0 if p in (1, 20, 40) else 1 for p in range(41)]
    ctx = rsv.Context(0)
    _check_case(rsv, ctx, [(9, 6, False), (8, 11, False)], 4, 41, mask, 7, 900, budget_cut=1)
    ctx.close()


def test_the_cap_is_trusted(rsv):
    """CAP_READ with one cap entry at a layer <= log_blowup overwritten: the overwritten node appears in d_witness where the
    plan puts it and nothing else changes, so untouched blocks are not recomputed."""
    spec, b, n, nq = [(5, 3, False), (4, 2, False)], 6, 2, 5
    ctx = rsv.Context(0)
    groups, q, gs, cap, base = _check_case(rsv, ctx, spec, b, n, None, nq, 1100, kind="any")
    top = 5 + b
    hits = 0
    for p in range(n):
        _, wit = D.plan(q[p], top)
        slot = sum(len(wit[l]) for l in range(top, b, -1))
        for l in range(b, 0, -1):
            for x in wit[l]:
                bad = cap.clone()
                bad[p, (1 << l) + x, 3] = 0x1234567
                got = _decommit_dev(rsv, ctx, gs, b, n, q, None, rsv.CAP_READ, cap=bad)
                want_w = base[2].copy()
                want_w[p, slot, 3] = 0x1234567
                assert np.array_equal(got[2], want_w), (p, l, x)
                assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and np.array_equal(got[3], base[3])
                slot += 1
                hits += 1
        assert slot == base[3][p]
    assert hits >= n  # 5 queries cannot cover the 8 nodes of layer 3: every proof misses a sibling at a layer <= 3
    ctx.close()


def test_device_refusals(rsv):
    """NULL pointers, n_queries 0 and 129, a bad mode, CAP_READ / CAP_WRITE without a buffer, misalignment, log_blowup out of
    range: the commitment's codes, nothing written."""
    import torch
    dev = torch.device(DEV)
    ctx = rsv.Context(0)
    cols = torch.zeros((1, 2, 16), dtype=torch.int32, device=dev)
    raw = torch.zeros(4096, dtype=torch.uint8, device=dev)
    b, nq = 2, 4
    g = {"log_size": 4, "d_cols": cols, "n_cols": 2}
    vcap, wcap = rsv.decommit_sizes([g], b, nq)
    mark = lambda shape: torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=dev)  # noqa: E731
    outs = {"d_values": mark((1, vcap)), "d_n_values": mark((1,)), "d_witness": mark((1, wcap, 8)), "d_n_witness": mark((1,))}
    cap = mark((1, 2 << b, 8))
    q = torch.zeros((1, nq), dtype=torch.int32, device=dev)

    def refused(code, groups=(g,), b=b, d_queries=q, nq=nq, **kw):
        args = dict(outs, **kw)
        with pytest.raises(rsv.RsvError) as e:
            ctx.decommit_tree(list(groups), 1, b, d_queries, nq, args["d_values"], args["d_n_values"], args["d_witness"], args["d_n_witness"],
                              cap_mode=args.get("cap_mode", 0), d_cap=args.get("d_cap"))
        assert e.value.code == code, (code, e.value.code)

    refused(-1, d_queries=None)
    for name in outs:
        refused(-1, **{name: None})
        refused(-2, **{name: raw[1:1025]})
    refused(-1, groups=[dict(g, d_cols=None)])
    refused(-1, cap_mode=rsv.CAP_READ)
    refused(-1, cap_mode=rsv.CAP_WRITE)
    refused(-2, cap_mode=3, d_cap=cap)
    refused(-2, cap_mode=rsv.CAP_WRITE, d_cap=raw[2:2050])
    refused(-2, nq=0)
    refused(-2, nq=129)
    refused(-2, b=0)
    refused(-2, b=17)
    refused(-2, groups=[g] * 9)
    refused(-2, groups=[dict(g, n_cols=0)])
    refused(-2, groups=[dict(g, log_size=29)])
    refused(-2, groups=[dict(g, d_cols=raw[1:])])
    refused(-2, d_queries=raw[1:17])
    roots = mark((1, 8))
    with pytest.raises(rsv.RsvError) as e:
        ctx.commit_tree([g], 1, b, roots, d_cap=raw[2:2050])
    assert e.value.code == -2
    ctx.synchronize()
    for t in list(outs.values()) + [cap, roots]:
        assert bool((t == 0x5A5A5A5A).all())
    ctx.decommit_tree([g], 1, b, q, nq, outs["d_values"], outs["d_n_values"], outs["d_witness"], outs["d_n_witness"], cap_mode=rsv.CAP_WRITE,
                      d_cap=cap)
    ctx.synchronize()
    # four times position 0: one leaf of two columns, one witness node per layer below the top = 4 + b
    assert int(outs["d_n_values"][0]) == 2 and int(outs["d_n_witness"][0]) == 4 + b and not bool((cap == 0x5A5A5A5A).any())
    ctx.close()
