"""rsv_commit_tree_dev / rsv_witness_commit_dev / rsv_witness_commit (`-m gpu`): trees 0, 1 and 2 of the next proof, their
Merkle roots and the transcript draws between them.  Against the REFERENCE for all 14 consecutive fixture pairs (with no
value borrowed from fixture K+1: the roots are its commitments[0..2], the draws its (z, alpha) and random_coeff, the sums
its stmt1, and the channel continued with its commitments[3] draws its OODS point), the coefficients and the LDE against
K+1's sampled and decommitted values, and bit for bit against the numpy restatement (tests/commit_ref.py, pinned to the
fixtures by tests/test_commit_host.py) on random trees."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import interaction_ref as R
from tests import oracle_binding as ob
from tests.chain_harness import CASES, DEV, chain, inputs_of, mask_dev, pin_id, pins, program_of, u32
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = C.P


def _want(dst):
    from oracle import recursion_circuit as rc
    nxt = read_proof(dst)
    d = rc.parse_proof(nxt)
    tr = ob.transcript_raw(nxt)
    return d, tr


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_chain_is_what_the_next_fixture_commits(rsv, pin):
    """The library alone, with K+1's log_blowup_factor and nothing else from K+1: roots = K+1's commitments[0..2], draws =
    its (z, alpha) and random_coeff, sums = its stmt1; the channel continued with commitments[3] draws its OODS point."""
    src, dst = pin["src"], pin["dst"]
    wp = program_of(rsv, pin)
    b = fixture_cfg(dst).log_blowup_factor
    ctx = rsv.Context(0)
    r = chain(rsv, ctx, wp, [read_proof(src)], inputs_of(src), b).numpy()
    ctx.close()
    d, tr = _want(dst)
    assert r["acc"][0] == 1 and r["ok"][0] == 1
    for t in range(3):
        assert r["roots"][0, t].tolist() == [int(x) for x in d.commitments[t]], t
    assert r["draws"][0].tolist() == tr[4:16].tolist()
    assert tuple(r["sums"][0, 0].tolist()) == tuple(d.plonk_total_sum) and tuple(r["sums"][0, 1].tolist()) == tuple(d.poseidon_total_sum)
    ch = C.Channel(ob, r["channel"][0, :8], int(r["channel"][0, 8]))
    assert not r["channel"][0, 9:].any()
    ch.mix([int(x) for x in d.commitments[3]])
    assert list(ch.draw()[0]) == tr[16:20].tolist()
    wp.close()


def test_host_form_equals_the_device_chain(rsv):
    pin = next(p for p in pins() if p["src"] == "level9-1.bin")
    wp = program_of(rsv, pin)
    src, dst = pin["src"], pin["dst"]
    b = fixture_cfg(dst).log_blowup_factor
    roots, draws, sums, ok, accept, _ = rsv.witness_commit([read_proof(src)], wp, b, inputs_of(src))
    d, tr = _want(dst)
    assert accept.tolist() == [1] and ok.tolist() == [1]
    assert roots[0].tolist() == [[int(x) for x in d.commitments[t]] for t in range(3)]
    assert draws[0].tolist() == tr[4:16].tolist()
    wp.close()


def _trees(wp, r, k):
    """The three trees' groups of proof k of a chain result, as (log, int64 columns) in commitment order."""
    lp, lq = wp.trace_sizes()
    ppre, qpre = wp.preprocessed()
    _, wops = wp.gates()
    ppre = ppre.copy()
    if len(wops):
        ppre[3, wops[:, 0]] = r["ops"][k]
    return [[(lp, ppre), (lq, qpre)], [(lp, r["plonk"][k]), (lq, r["poseidon"][k])], [(lp, r["int_plonk"][k]), (lq, r["int_poseidon"][k])]]


def _commit_dev(rsv, ctx, groups, b, n=1, coeffs=False, lde=False, mask=None, shared=()):
    """Context.commit_tree of numpy groups [(log, uint32[n or 1, cols, 2^log])] -> (roots, [coeffs], [lde])."""
    import torch
    dev = torch.device(DEV)
    gs, cf, ld = [], [], []
    for i, (log, cols) in enumerate(groups):
        cols = np.ascontiguousarray(np.asarray(cols, dtype=np.int64) % P, dtype=np.uint32)
        if cols.ndim == 2:
            cols = cols[None]
        t = torch.from_numpy(cols.view(np.int32)).to(dev)
        nc = cols.shape[1]
        g = {"log_size": log, "d_cols": t, "n_cols": nc, "proof_stride": 0 if i in shared else nc << log}
        if coeffs:
            g["d_coeffs"] = torch.full((n, nc, 1 << log), -1, dtype=torch.int32, device=dev)
            cf.append(g["d_coeffs"])
        if lde:
            g["d_lde"] = torch.full((n, nc, 1 << (log + b)), -1, dtype=torch.int32, device=dev)
            ld.append(g["d_lde"])
        gs.append(g)
    d_roots = torch.full((n, 8), -1, dtype=torch.int32, device=dev)
    d_mask = mask_dev(mask)
    ctx.commit_tree(gs, n, b, d_roots, d_mask)
    ctx.synchronize()
    return u32(d_roots), [u32(x) for x in cf], [u32(x) for x in ld]


@pytest.mark.parametrize("src", ["level2-1.bin", "level6-1.bin", "level9-1.bin"])
def test_coefficients_give_the_sampled_values(rsv, src):
    """d_coeffs of the three trees evaluated at K+1's OODS point (and at the previous-row point where the mask asks for it)
    = K+1's 134 sampled values of trees 0-2; the roots from rsv_commit_tree_dev = the chain's."""
    pin = next(p for p in pins() if p["src"] == src)
    wp = program_of(rsv, pin)
    dst = pin["dst"]
    b = fixture_cfg(dst).log_blowup_factor
    ctx = rsv.Context(0)
    r = chain(rsv, ctx, wp, [read_proof(src)], inputs_of(src), b).numpy()
    d, tr = _want(dst)
    oods = (tuple(int(x) for x in tr[20:24]), tuple(int(x) for x in tr[24:28]))
    for t, groups in enumerate(_trees(wp, r, 0)):
        roots, cf, _ = _commit_dev(rsv, ctx, groups, b, coeffs=True)
        assert roots[0].tolist() == r["roots"][0, t].tolist(), t
        got = []
        for (log, _), co in zip(groups, cf):
            for k in range(co.shape[1]):
                if t == 2 and k >= 4:
                    got.append([C.eval_at_point(co[0, k], log, R.prev_row_point(oods, log)), C.eval_at_point(co[0, k], log, oods)])
                else:
                    got.append([C.eval_at_point(co[0, k], log, oods)])
        want = [[tuple(v) for v in col] for col in d.sampled_values[t]]
        assert got == want, (t, [k for k in range(len(want)) if got[k] != want[k]])
    ctx.close()
    wp.close()


@pytest.mark.parametrize("src", ["recursive_proof_16_15.bin", "level2-1.bin"])
def test_lde_at_the_query_positions(rsv, src):
    """d_lde of the three trees at K+1's query positions = the values K+1 decommits (SinglePathMerkleProof::columns)."""
    pin = next(p for p in pins() if p["src"] == src)
    wp = program_of(rsv, pin)
    dst = pin["dst"]
    b = fixture_cfg(dst).log_blowup_factor
    ctx = rsv.Context(0)
    r = chain(rsv, ctx, wp, [read_proof(src)], inputs_of(src), b).numpy()
    nxt = read_proof(dst)
    cols = ob.trace_cols(nxt, inputs_of(dst))
    qM, M = C.query_positions(nxt, ob)
    for t, groups in enumerate(_trees(wp, r, 0)):
        roots, _, ld = _commit_dev(rsv, ctx, groups, b, lde=True)
        assert roots[0].tolist() == r["roots"][0, t].tolist(), t
        layers = {}
        for (log, _), e in zip(groups, ld):
            layers[log + b] = e[0] if log + b not in layers else np.concatenate([layers[log + b], e[0]])
        top = max(layers)
        for j, q in enumerate(qM):
            got = C.decommitted(layers, int(q) >> (M - top))
            assert got == cols[t, j, :len(got)].tolist(), (t, j)
    ctx.close()
    wp.close()


def _random_case(rsv, ctx, spec, b, n, mask, seed, label):
    """One random tree of CASES / GLOBAL_CASES on ctx: roots, d_coeffs and d_lde = the restatement; a masked proof gets
    zeros."""
    rng = np.random.default_rng(seed)
    groups = [(log, rng.integers(0, P, (1 if sh else n, nc, 1 << log))) for log, nc, sh in spec]
    shared = {i for i, (_, _, sh) in enumerate(spec) if sh}
    roots, cf, ld = _commit_dev(rsv, ctx, groups, b, n=n, coeffs=True, lde=True, mask=mask, shared=shared)
    for p in range(n):
        if mask is not None and not mask[p]:
            assert not roots[p].any() and all(not c[p].any() for c in cf) and all(not e[p].any() for e in ld), (label, p)
            continue
        mine = [(log, cols[0 if i in shared else p]) for i, (log, cols) in enumerate(groups)]
        for i, ((log, cols), co, e) in enumerate(zip(mine, cf, ld)):
            assert np.array_equal(co[p], C.interpolate(cols, log)), (label, p, i)
            assert np.array_equal(e[p], C.evaluate(co[p], log, log + b)), (label, p, i)
        assert roots[p].tolist() == C.commit(mine, b, ob).tolist(), (label, p)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_commit_tree_bit_for_bit(rsv, case):
    """Random trees: roots, d_coeffs and d_lde = the restatement; a masked proof gets zeros."""
    spec, b, n, mask = CASES[case]
    ctx = rsv.Context(0)
    _random_case(rsv, ctx, spec, b, n, mask, 100 + case, case)
    ctx.close()


GLOBAL_CASES = [  # as CASES: around CM_LDS_LOG = 12 (layers m >= 12 run in k_cm_fft_layer) and at the driver's limits
    ([(11, 2, False)], 3, 2, None),
    ([(12, 2, False)], 2, 2, None),
    ([(13, 2, False)], 3, 2, None),  # one global layer each way, the forward one reading the coefficients through CmSrc
    ([(14, 1, False)], 2, 3, None),  # forward table of 2^16 again (cached by the case above)
    ([(16, 1, False)], 1, 1, None),  # four global layers; the inverse table of 2^16
    ([(13, 1, False), (15, 2, False)], 2, 2, None),  # two global depths feeding one hash layer each
    ([(14, 2, True), (9, 3, False)], 2, 4, [1, 0, 1, 0]),  # a masked shared group (proof_stride 0) through the global layers
    ([(2, 3, False)], 16, 2, None),  # RSV_MAX_LOG_BLOWUP: 2^16 block subtrees, 16 node layers above them
    ([(0, 2, False)], 16, 2, [0, 1]),
    ([(3, 3, False), (3, 6, False), (2, 7, False), (3, 1, False), (2, 2, False), (3, 4, False), (4, 9, False), (2, 5, False)], 3, 2,
     None),  # RSV_MAX_COMMIT_GROUPS, interleaved sizes: 8-word chunks of k_cm_hash_layer across group boundaries
    ([(5, 3, False), (4, 2, False), (5, 6, False)], 3, 3, [1, 1, 0]),  # equal logs apart: joined in group order
]


def test_commit_tree_global_passes_and_limits(rsv):
    """GLOBAL_CASES in one Context (the twiddle tables cached by a case serve the later ones): logs 11 to 16 across the LDS /
    global-pass boundary, two global depths in one tree, a masked shared log-14 group, log_blowup 16 at logs 2 and 0, 8
    groups, equal logs out of order.  Roots, d_coeffs and d_lde = the restatement, element by element."""
    ctx = rsv.Context(0)
    for case, (spec, b, n, mask) in enumerate(GLOBAL_CASES):
        _random_case(rsv, ctx, spec, b, n, mask, 300 + case, case)
    ctx.close()


def test_workspace_groups_and_one_proof(rsv):
    """A batch cut into passes (fewer blocks, then fewer proofs) under a 1 MB workspace budget equals the uncut batch and
    the restatement; n = 1 equals proof 0 of the batch."""
    rng = np.random.default_rng(9)
    n, b = 40, 4
    groups = [(9, rng.integers(0, P, (n, 6, 1 << 9))), (8, rng.integers(0, P, (n, 11, 1 << 8)))]
    ctx = rsv.Context(0)
    whole, _, _ = _commit_dev(rsv, ctx, groups, b, n=n)
    ctx.set_option("ws_budget_mb", 1)
    cut, _, _ = _commit_dev(rsv, ctx, groups, b, n=n)
    one, _, _ = _commit_dev(rsv, ctx, [(log, c[:1]) for log, c in groups], b, n=1)
    ctx.close()
    assert np.array_equal(whole, cut)
    assert np.array_equal(one[0], whole[0])
    for p in (0, 17, 39):
        assert whole[p].tolist() == C.commit([(log, c[p]) for log, c in groups], b, ob).tolist(), p


def test_workspace_cut_with_caller_owned_outputs(rsv):
    """d_coeffs and d_lde given, a mask, 41 proofs at b = 3 of a log-13 group, a shared log-9 group and a log-10 group.  The
    workspace is then the node layers alone, about P nb 384 KiB: a 5 MB budget cuts it to one block per pass (nb = 1 < 2^b)
    and to P = 11 proofs per pass (41 -> 21 -> 11), so four passes of 11, 11, 11 and a short last one of 8, each reaching
    its outputs at p0 and blk0 offsets.  Masked proofs sit in the first, a middle and the last pass.  Every element of the
    roots, d_coeffs and d_lde equals the uncut run; sampled proofs equal the restatement; masked proofs are all zeros."""
    rng = np.random.default_rng(41)
    n, b = 41, 3
    spec = [(13, 2, False), (9, 3, True), (10, 4, False)]
    groups = [(log, rng.integers(0, P, (1 if sh else n, nc, 1 << log))) for log, nc, sh in spec]
    shared = {1}
    mask = [0 if p in (1, 20, 39) else 1 for p in range(n)]
    ctx = rsv.Context(0)
    whole = _commit_dev(rsv, ctx, groups, b, n=n, coeffs=True, lde=True, mask=mask, shared=shared)
    ctx.set_option("ws_budget_mb", 5)
    cut = _commit_dev(rsv, ctx, groups, b, n=n, coeffs=True, lde=True, mask=mask, shared=shared)
    ctx.close()
    roots, cf, ld = whole
    assert np.array_equal(cut[0], roots)
    for i in range(len(spec)):
        assert np.array_equal(cut[1][i], cf[i]), i
        assert np.array_equal(cut[2][i], ld[i]), i
    for p in (1, 20, 39):
        assert not roots[p].any() and all(not c[p].any() for c in cf) and all(not e[p].any() for e in ld), p
    for p in (0, 10, 11, 33, 40):
        mine = [(log, cols[0 if i in shared else p]) for i, (log, cols) in enumerate(groups)]
        for i, ((log, cols), co, e) in enumerate(zip(mine, cf, ld)):
            assert np.array_equal(co[p], C.interpolate(cols, log)), (p, i)
            assert np.array_equal(e[p], C.evaluate(co[p], log, log + b)), (p, i)
        assert roots[p].tolist() == C.commit(mine, b, ob).tolist(), p


def test_mixed_batch_with_a_rejected_proof(rsv):
    """Five proofs of one shape, the third tampered (rejected): it gets zeros everywhere and d_ok = 0; every output element
    of the others is written and equals its solo run."""
    pin = next(p for p in pins() if p["src"] == "level9-1.bin")
    wp = program_of(rsv, pin)
    src = pin["src"]
    b = fixture_cfg(pin["dst"]).log_blowup_factor
    proof = read_proof(src)
    batch = [proof, proof, ob.tamper(proof, 5), proof, proof]
    ctx = rsv.Context(0)
    r = chain(rsv, ctx, wp, batch, inputs_of(src), b).numpy()
    solo = chain(rsv, ctx, wp, [proof], inputs_of(src), b).numpy()
    ctx.close()
    assert r["acc"].tolist() == [1, 1, 0, 1, 1] and r["ok"].tolist() == [1, 1, 0, 1, 1]
    for key in ("roots", "draws", "int_plonk", "int_poseidon", "sums", "channel"):
        assert not r[key][2].any(), key
        for k in (0, 1, 3, 4):
            assert np.array_equal(r[key][k], solo[key][0]), (key, k)
    wp.close()


def test_chain_under_a_small_workspace_budget(rsv):
    """The batch of test_mixed_batch_with_a_rejected_proof (the level10 shape, 2^16 / 2^15 rows at b = 8) under a 200 MB
    budget: each of the three commit_tree calls keeps its five proofs but cuts its 256 blocks into passes of nb = 2 (trees 0
    and 1) or nb = 4 (tree 2, about 16 MB of coefficients + 31 MB per block), with d_accept, then ok, as the mask.  Every
    output, ok included, is bit-identical to the default-budget run."""
    pin = next(p for p in pins() if p["src"] == "level9-1.bin")
    wp = program_of(rsv, pin)
    src = pin["src"]
    b = fixture_cfg(pin["dst"]).log_blowup_factor
    assert wp.trace_sizes() == (16, 15) and b == 8
    proof = read_proof(src)
    batch = [proof, proof, ob.tamper(proof, 5), proof, proof]
    ctx = rsv.Context(0)
    whole = chain(rsv, ctx, wp, batch, inputs_of(src), b).numpy()
    ctx.set_option("ws_budget_mb", 200)
    cut = chain(rsv, ctx, wp, batch, inputs_of(src), b).numpy()
    ctx.close()
    assert whole["ok"].tolist() == [1, 1, 0, 1, 1]
    for key in ("roots", "draws", "int_plonk", "int_poseidon", "sums", "channel", "ok"):
        assert np.array_equal(cut[key], whole[key]), key
    assert not whole["roots"][2].any() and whole["roots"][0].any()
    wp.close()


def test_device_refusals(rsv):
    """RSV_E_SIZE with nothing written for a misaligned pointer, log_blowup 0 or above the limit, log + b above
    RSV_MAX_LOG_SIZE, too many groups; RSV_E_NULL for missing columns."""
    import torch
    dev = torch.device(DEV)
    ctx = rsv.Context(0)
    cols = torch.zeros((1, 2, 16), dtype=torch.int32, device=dev)
    raw = torch.zeros(4 * 32 + 8, dtype=torch.uint8, device=dev)
    roots = torch.full((1, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)

    def refused(code, groups, b=2, d_roots=roots):
        with pytest.raises(rsv.RsvError) as e:
            ctx.commit_tree(groups, 1, b, d_roots)
        assert e.value.code == code

    g = {"log_size": 4, "d_cols": cols, "n_cols": 2}
    refused(-2, [g], b=0)
    refused(-2, [g], b=17)
    refused(-2, [dict(g, log_size=29)], b=2)
    refused(-2, [g] * 9)
    refused(-2, [dict(g, n_cols=0)])
    refused(-1, [dict(g, d_cols=None)])
    refused(-2, [dict(g, d_cols=raw[1:])])
    refused(-2, [g], d_roots=raw[2:34])
    ctx.synchronize()
    assert bool((roots == 0x5A5A5A5A).all())
    ctx.commit_tree([g], 1, 2, roots)
    ctx.synchronize()
    ctx.close()
