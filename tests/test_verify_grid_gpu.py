"""Genuine proofs at the configurations no fixture has (`-m gpu`): the grid of tests/verify_grid.py, every proof made once per
run by rsv.Chain, certified by the C oracle (tests/oracle_binding, which reads the configuration from its argument and is
pinned to the reference by its KAT and the fixtures) and then put through rsv_verify_batch_dev's accepting path: one proof
per call, every forced kernel form in mixed batches, the values k_query computes, the paths and the flow, batches one proof
past a k_query workgroup, mutants behind the proof of work, and all of it as one job through one context.  The reference in
every assert is the oracle; every comparison is exact."""
import time

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import verify_grid as G
from tests.chain_harness import DEV, FILL
from tests.conftest import load_manifest, read_proof, fixture_cfg

pytestmark = pytest.mark.gpu
POINTS = list(G.POINTS)
S_POINTS = [p for p in POINTS if p[0] not in G.R_SRCS]
R_POINTS = [p for p in POINTS if p[0] in G.R_SRCS]
RSV_E_SIZE = -2
# the points whose geometry the mutants and the slot batches are built at
MUTANT_POINTS = [("S1", 2, 1, 0, 1), ("S1", 2, 1, 0, 3), ("S1", 2, 1, 0, 33), ("S1", 2, 1, 0, 128), ("R", 2, 1, 8, 128),
                 ("S2", 2, 2, 4, 6), ("S2", 2, 2, 5, 6), ("R", 2, 1, 12, 16)]
SLOT_POINTS = [("S1", 2, 1, 0, 3), ("S1", 2, 1, 0, 5), ("S1", 2, 1, 0, 33), ("S1", 2, 1, 0, 128), ("R", 2, 1, 8, 128)]
assert set(MUTANT_POINTS) | set(SLOT_POINTS) <= set(POINTS)


class Item:
    def __init__(self, point, proof, cfg, inputs, seconds):
        self.point, self.proof, self.cfg, self.inputs, self.seconds = point, proof, cfg, inputs, seconds
        self.lp, self.lq = (int(x) for x in np.frombuffer(proof[:8], np.uint32))
        self.M, self.A, self.B, self.n_inner = G.sizes_of(self.lp, self.lq, point)
        self.nq = point[4]
        self.G = max(self.nq, 4)


@pytest.fixture(scope="module")
def ctx(rsv):
    c = rsv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def programs(rsv):
    p = G.Programs(rsv)
    yield p
    p.close()


def _generate(rsv, ctx, programs, points):
    out = {}
    for point in points:
        t0 = time.perf_counter()
        proof, cfg, inputs = G.generate(rsv, ctx, point, programs)
        out[point] = Item(point, proof, cfg, inputs, time.perf_counter() - t0)
        print("generated %-28s %7.1f ms %8d bytes" % (G.point_id(point), 1e3 * out[point].seconds, len(proof)))
    return out


@pytest.fixture(scope="module")
def grid(rsv, ctx, programs):
    """Every point's genuine proof, made once and kept in memory."""
    G.generate(rsv, ctx, POINTS[0], programs)                # (the first call of a process pays for loading the kernels)
    return _generate(rsv, ctx, programs, POINTS)


@pytest.fixture(scope="module")
def grid0(rsv, ctx, programs):
    """The mutants' points made again with pow_bits = 0: a mutated transcript word no longer stops at the proof of work."""
    return _generate(rsv, ctx, programs, [(p[0], 0) + p[2:] for p in MUTANT_POINTS])


def _pairs(acc, reason):
    return list(zip(np.asarray(acc).tolist(), np.asarray(reason).tolist()))


def _verify_dev(rsv, ctx, proofs, cfgs, inputs):
    """One rsv_verify_batch_dev call through `ctx` -> [(accept, reason)]; the outputs are prefilled with 7."""
    import torch
    n = len(proofs)
    blob, offsets = rsv.pack(proofs)
    d_blob = torch.from_numpy(blob.copy()).to(DEV)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(DEV)
    d_acc = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    d_reason = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    ctx.verify_batch(d_blob, d_off, n, d_acc, d_reason, cfg=cfgs, inputs=inputs)
    ctx.synchronize()
    return _pairs(d_acc.cpu().numpy(), d_reason.cpu().numpy())


# ---------------------------------------------------------------- 1, 2. certified by the oracle, accepted one per call
@pytest.mark.parametrize("point", POINTS, ids=G.point_id)
def test_oracle_certifies_the_proof(grid, point):
    """A failure here is a prover bug, or an oracle bug, at a configuration nobody has proved before."""
    it = grid[point]
    w = np.frombuffer(it.proof[:56], np.uint32)
    assert w[10:14].tolist() == list(point[1:]) and ob.proof_layout(it.proof)["n_inner"] == it.n_inner
    assert _pairs(*ob.verify_batch([it.proof], it.cfg, it.inputs)) == [(1, 0)]


@pytest.mark.parametrize("point", POINTS, ids=G.point_id)
def test_one_proof_per_call_default_forms(rsv, grid, point):
    """A single proof takes the row forms by itself: G = 32 is their last geometry, 33 the first that falls back."""
    it = grid[point]
    assert _pairs(*rsv.verify_batch([it.proof], it.cfg, it.inputs)) == [(1, 0)]


# ---------------------------------------------------------------- 3. every forced form, mixed batches
def _chunks(points, size=16):
    return [points[k:k + size] for k in range(0, len(points), size)]


@pytest.fixture(scope="module")
def calls(grid):
    """The grid as mixed batches of at most 16 configurations: the S points (they share their public inputs) in table
    order, R in a call of its own; behind every genuine proof a copy with one bit flipped.  -> [(proofs, cfgs, inputs, the
    oracle's [(accept, reason)], the points)]."""
    out = []
    for k, points in enumerate(_chunks(S_POINTS) + _chunks(R_POINTS)):
        proofs, cfgs = [], []
        for j, p in enumerate(points):
            proofs += [grid[p].proof, ob.tamper(grid[p].proof, 16 * k + j)]
            cfgs += [grid[p].cfg] * 2
        inputs = grid[points[0]].inputs
        assert all(grid[p].inputs == inputs for p in points)
        want = _pairs(*ob.verify_batch(proofs, cfgs, inputs))
        assert want[0::2] == [(1, 0)] * len(points) and all(a == 0 for a, _ in want[1::2])
        out.append((proofs, cfgs, inputs, want, points))
    return out


FORMS = [{}]
FORMS += [{"tree_pace": v} for v in ("paced", "unpaced", "row16")]
FORMS += [{"query_form": v} for v in ("lane", "row")]
FORMS += [{"transcript_form": "lane"}, {"transcript_form": "row"}, {"transcript_form": "row", "transcript_split": "whole"},
          {"transcript_form": "row", "transcript_split": "split"}]
FORMS += [{"oods_form": v} for v in ("lane", "row")]
FORMS += [{"qconst_form": v} for v in ("lane", "row")]
FORMS += [{"plan_form": v} for v in ("serial", "parallel")]
FORMS += [{"tree_cap": v} for v in ("on", "off")]
FORMS += [{"cap_top": v} for v in ("on", "off")]
FORMS += [{"cap_top": "on", "cap_mid": v} for v in ("auto", "on", "off")]   # (the middle kernel feeds k_cap_top)
FORMS += [{"critical_chain": v} for v in ("on", "off")]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: ",".join("%s=%s" % kv for kv in f.items()) or "default")
def test_every_forced_form_on_the_whole_grid(rsv, knobs, grid, calls, form):
    """One family of forms at a time against the default, the whole grid in mixed batches: verdicts and reasons are the
    oracle's.  The first call mixes buckets of G > 32 with buckets of G <= 32, so that under row16 (and by default) the
    call-wide fallback from the row forms runs with genuine proofs on both sides of it."""
    gs = [grid[p].G for p in calls[0][4]]
    assert max(gs) > 32 and min(gs) <= 32 and 32 in gs and 33 in gs
    for name, value in form.items():
        knobs.set(name, value)
    for proofs, cfgs, inputs, want, points in calls:
        got = _pairs(*rsv.verify_batch(proofs, cfgs, inputs))
        assert got == want, [(G.point_id(points[i // 2]), i % 2, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    # only buckets the row forms take: nothing falls back
    row = [i for i, p in enumerate(calls[0][4]) if grid[p].G <= 32]
    proofs, cfgs = [calls[0][0][2 * i + h] for i in row for h in (0, 1)], [calls[0][1][2 * i + h] for i in row for h in (0, 1)]
    assert _pairs(*rsv.verify_batch(proofs, cfgs, calls[0][2])) == [calls[0][3][2 * i + h] for i in row for h in (0, 1)]


# ---------------------------------------------------------------- 4. values, not only verdicts
QUERY_FORMS = {"lane, one stream": {"tree_pace": "paced", "query_form": "lane", "critical_chain": "on"},
               "lane, two streams": {"tree_pace": "paced", "query_form": "lane", "critical_chain": "off"},
               "row": {"tree_pace": "row16", "query_form": "row"}}
VALUE_CASES = [(p, f) for p in POINTS for f in QUERY_FORMS if f != "row" or max(p[4], 4) <= 32]


@pytest.mark.parametrize("point, form", VALUE_CASES, ids=lambda v: G.point_id(v) if isinstance(v, tuple) else v)
def test_query_values_match_oracle(rsv, grid, point, form):
    """k_query's DEEP answers, first-layer folds, every inner layer's input and the last-layer evaluation, word for word,
    at each geometry.  d_query_values is a path output: below four queries the call is refused (include/rsv.h)."""
    import torch
    it = grid[point]
    n = 2
    blob, offsets = rsv.pack([it.proof] * n)
    d_blob = torch.from_numpy(blob.copy()).to(DEV)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(DEV)
    d_acc = torch.zeros(n, dtype=torch.uint8, device=DEV)
    d_qv = torch.full((n, it.nq, 4 * (8 + it.n_inner)), -1, dtype=torch.int32, device=DEV)
    c = rsv.Context(0)
    try:
        for name, value in QUERY_FORMS[form].items():
            c.set_option(name, value)
        call = lambda: c.verify_hints(d_blob, d_off, n, d_acc, None, cfg=it.cfg, inputs=it.inputs, shape=(it.nq, it.M, it.n_inner),  # noqa: E731
                                      d_query_values=d_qv)
        if it.nq < 4:
            with pytest.raises(rsv.RsvError) as e:
                call()
            assert e.value.code == RSV_E_SIZE
            return
        call()
        c.synchronize()
        assert d_acc.cpu().tolist() == [1] * n
        want = ob.query_dump(it.proof, it.inputs)
        got = d_qv.cpu().numpy().view(np.uint32)
        assert want.shape == got[0].shape
        for k in range(n):
            assert np.array_equal(got[k], want), (k, np.argwhere(got[k] != want)[:4].tolist())
        ni = it.n_inner
        assert np.array_equal(want[:, 24 + 4 * ni:28 + 4 * ni], want[:, 28 + 4 * ni:32 + 4 * ni])   # the accepting side of FRI_LAST
    finally:
        c.close()


# ---------------------------------------------------------------- 5. paths and flow
@pytest.mark.parametrize("trees", ["paced", "row16"])
@pytest.mark.parametrize("point", POINTS, ids=G.point_id)
def test_paths_and_flow_match_oracle(rsv, knobs, grid, point, trees):
    it = grid[point]
    nq, M, ni = it.nq, it.M, it.n_inner
    knobs.set("tree_pace", trees)
    if nq < 4:
        # the path outputs are laid out by G = max(n_queries, 4) lanes and are refused below four (include/rsv.h); the flow is
        # laid out by n_queries and is not
        for call in (lambda: rsv.trace_paths([it.proof], it.cfg, nq, M, it.inputs), lambda: rsv.fri_paths([it.proof], it.cfg, nq, M, ni, it.inputs)):
            with pytest.raises(rsv.RsvError) as e:
                call()
            assert e.value.code == RSV_E_SIZE
    else:
        _paths_match_oracle(rsv, it)
    want = ob.poseidon_flow(it.proof, it.inputs)
    cnt = rsv.poseidon_flow_count(it.lp, it.lq, it.cfg)
    assert cnt == len(want)
    flow, swap, count, acc, reason = rsv.poseidon_flow([it.proof], it.cfg, cnt + 3, it.inputs)
    assert _pairs(acc, reason) == [(1, 0)] and count.tolist() == [cnt]
    assert np.array_equal(flow[0, :cnt], want[:, :32]), int(np.nonzero((flow[0, :cnt] != want[:, :32]).any(axis=1))[0][0])
    assert np.array_equal(swap[0, :cnt], want[:, 32].astype(np.uint8)) and not flow[0, cnt:].any() and not swap[0, cnt:].any()


def _paths_match_oracle(rsv, it):
    nq, M, ni = it.nq, it.M, it.n_inner
    osib, opos, depth = ob.trace_paths(it.proof, nq, M, it.inputs)
    sib, pos, acc, reason = rsv.trace_paths([it.proof], it.cfg, nq, M, it.inputs)
    assert _pairs(acc, reason) == [(1, 0)] and np.array_equal(pos[0], opos)
    for t in range(4):
        d = int(depth[t])
        assert np.array_equal(sib[0, t, :, :d, :], osib[t, :, :d, :]), t
    osib, ocols = ob.fri_paths(it.proof, nq, M, 1 + ni, it.inputs)
    sib, cols, acc, reason = rsv.fri_paths([it.proof], it.cfg, nq, M, ni, it.inputs)
    assert _pairs(acc, reason) == [(1, 0)] and np.array_equal(cols[0], ocols)
    for s in range(1 + ni):
        d = M if s == 0 else M - s
        assert np.array_equal(sib[0, s, :, :d - 1, :], osib[s, :, :d - 1, :]), s


# ---------------------------------------------------------------- the defect the grid found
@pytest.mark.parametrize("shape, b, ll", [("S1", 1, 5), ("S2", 2, 7)])
def test_chain_refuses_a_last_layer_its_smallest_column_folds_into(rsv, ctx, programs, shape, b, ll):
    """log_last = min(lp, lq) - 1: the chain said ok and wrote a proof that the oracle and the library both rejected with
    RSV_R_FRI_LAST (test_oracle_certifies_the_proof, on the table's first layout).  The smallest column would meet no inner
    layer, so no accepting proof exists; rsv_witness_fri_dev refuses, while rsv_fri_sizes still answers the arithmetic."""
    prog, built = programs.of(shape), programs.built[shape]
    lp, lq = prog.trace_sizes()
    assert min(lp, lq) == ll + 1 and not G.provable(lp, lq, (shape, 2, b, ll, 6)) and rsv.fri_sizes(lp, lq, b, ll)["n_inner"] >= 1
    ch = rsv.Chain(ctx, prog, 1, b, log_last=ll, fill=FILL, caps=True, device=DEV)
    ch.load(built.variables[None], built.unbound_flow()[None], None, check=True)
    for stage in ("trace", "commit", "tree3", "sample"):
        getattr(ch, stage)()
    with pytest.raises(rsv.RsvError) as e:
        ch.fri()
    assert e.value.code == RSV_E_SIZE


# ---------------------------------------------------------------- 6. slot geometry
@pytest.mark.parametrize("point", SLOT_POINTS, ids=G.point_id)
def test_one_proof_past_a_query_workgroup(rsv, ctx, grid, point):
    """256 // G + 1 copies, one more proof than a k_query workgroup holds, the middle one with a byte of its first queried
    value flipped; a second pass through the same context, its workspaces grown, says the same."""
    it = grid[point]
    n = 256 // it.G + 1
    pos = next(p for p, _n, what in ob.proof_layout(it.proof)["prefixes"] if what == "queried_values[0]")
    bad = bytearray(it.proof)
    bad[4 * (pos + 2)] ^= 1
    proofs = [it.proof] * n
    proofs[n // 2] = bytes(bad)
    want = _pairs(*ob.verify_batch(proofs, it.cfg, it.inputs))
    assert [a for a, _ in want] == [0 if k == n // 2 else 1 for k in range(n)]
    for _ in range(2):
        assert _verify_dev(rsv, ctx, proofs, it.cfg, it.inputs) == want


# ---------------------------------------------------------------- 7. mutants at the new geometries
R_MERKLE_T0, R_FRI_FIRST, R_FRI_INNER = 6, 10, 11          # rsv_reason: MERKLE_T0..T3 = 6..9 (include/rsv.h)


@pytest.fixture(scope="module")
def corpus(grid0):
    """Per proof made under pow_bits = 0: itself, tests.mutants.mutants_of(proof, rng, 40) and 120 random byte flips placed
    as in test_gpu_parity.test_mutants_behind_the_proof_of_work_match_oracle.  -> [(proofs, cfgs, inputs, the oracle's
    [(accept, reason)], the indices of the genuine proofs)], the S proofs in one batch, R's in another."""
    from tests.mutants import mutants_of
    rng = np.random.default_rng(23)
    out = []
    for shapes in (("S1", "S2", "S3"), tuple(G.R_SRCS)):
        proofs, cfgs, genuine, inputs = [], [], [], None
        for point, it in grid0.items():
            if point[0] not in shapes:
                continue
            inputs = it.inputs
            proof = it.proof
            n_head = 4 * ob.proof_layout(proof)["nonce_word"]    # everything in front of the nonce is absorbed by the transcript
            mut = [proof] + mutants_of(proof, rng, 40)
            for k in range(120):
                b = bytearray(proof)
                for _ in range(1 + k % 3):
                    at = int(rng.integers(68, 132)) if k % 4 == 1 else int(rng.integers(68, n_head)) if k % 2 else int(rng.integers(0, len(b)))
                    b[at] = int(rng.integers(0, 256))
                mut.append(bytes(b))
            genuine.append(len(proofs))
            proofs += mut
            cfgs += [it.cfg] * len(mut)
        t0 = time.perf_counter()
        want = _pairs(*ob.verify_batch(proofs, cfgs, inputs))
        print("oracle: %d proofs of %s in %.1f s" % (len(proofs), "/".join(shapes), time.perf_counter() - t0))
        out.append((proofs, cfgs, inputs, want, genuine))
    return out


def test_mutant_corpus_reaches_every_stage(corpus):
    """Checked on the ORACLE's output, so that the GPU tests below cannot pass by rejecting everything at the parser."""
    want = [w for call in corpus for w in call[3]]
    counts = np.bincount([r for _, r in want], minlength=16)
    print("oracle's reasons over the corpus (reason: count):", {int(r): int(c) for r, c in enumerate(counts) if c})
    assert all(call[3][g] == (1, 0) for call in corpus for g in call[4])
    assert counts[2] == 0                                   # pow_bits = 0: nothing stops at the proof of work
    assert counts[3] > 0 and counts[4] > 0                  # logup, OODS
    assert all(counts[r] > 0 for r in range(R_MERKLE_T0, R_MERKLE_T0 + 4)), counts.tolist()
    assert counts[R_FRI_FIRST] > 0 and counts[R_FRI_INNER] > 0, counts.tolist()


@pytest.mark.parametrize("which", [0, 1], ids=["S", "R"])
def test_mutants_at_the_new_geometries_match_oracle(rsv, corpus, which):
    proofs, cfgs, inputs, want, genuine = corpus[which]
    got = _pairs(*rsv.verify_batch(proofs, cfgs, inputs))
    diff = [i for i in range(len(want)) if got[i] != want[i]]
    assert not diff, [(i, cfgs[i].n_queries, cfgs[i].log_last_layer_degree_bound, got[i], want[i]) for i in diff[:10]]
    assert all(got[g] == (1, 0) for g in genuine)


# ---------------------------------------------------------------- 8. all of it as one job
def test_everything_as_one_job_through_one_context(rsv, ctx, grid, grid0):
    """Every generated proof and the accepted fixtures, shuffled, each under its own configuration, through one context,
    twice.  A call shares its public inputs and holds at most 16 configurations, so the job is cut by input set and then
    by configuration count."""
    jobs = {}
    for it in list(grid.values()) + list(grid0.values()):
        jobs.setdefault(repr(it.inputs), (it.inputs, []))[1].append((it.proof, it.cfg))
    fixtures = [e for e in load_manifest() if e["expect"] == "ok"]
    assert len(fixtures) == 15
    for e in fixtures:
        inputs = [(i, tuple(v)) for i, v in e["inputs"]]
        jobs.setdefault(repr(inputs), (inputs, []))[1].append((read_proof(e["file"]), fixture_cfg(e["file"])))
    rng = np.random.default_rng(29)
    key = lambda c: (c.pow_bits, c.log_blowup_factor, c.log_last_layer_degree_bound, c.n_queries)  # noqa: E731
    calls = []
    for inputs, members in jobs.values():
        members = [members[i] for i in rng.permutation(len(members))]
        cur, seen = [], set()
        for proof, cfg in members:
            if key(cfg) not in seen and len(seen) == rsv.MAX_CFGS:
                calls.append((inputs, cur))
                cur, seen = [], set()
            seen.add(key(cfg))
            cur.append((proof, cfg))
        calls.append((inputs, cur))
    assert sum(len(c) for _, c in calls) == len(grid) + len(grid0) + 15 and len(calls) >= 5
    wants = [_pairs(*ob.verify_batch([p for p, _ in c], [k for _, k in c], inputs)) for inputs, c in calls]
    assert all(w == [(1, 0)] * len(w) for w in wants)
    for _ in range(2):
        for (inputs, c), want in zip(calls, wants):
            assert _verify_dev(rsv, ctx, [p for p, _ in c], [k for _, k in c], inputs) == want
