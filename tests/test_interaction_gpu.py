"""rsv_witness_interaction / rsv_witness_interaction_dev (`-m gpu`): tree 2 of the next proof, the interaction (logup)
columns, and its two claimed sums.  Against the REFERENCE for all 14 consecutive fixture pairs (with fixture K+1's own
lookup elements, the sums are K+1's stmt1 and the 16 columns give K+1's 24 tree-2 sampled values), and bit for bit
against the numpy restatement (tests/interaction_ref.py, pinned to the fixtures by tests/test_interaction_host.py) fed
with the GPU's own trace columns: a mixed batch with per-proof lookup elements and rejected proofs, both variable layouts,
a five-copy program, one proof, a crafted zero denominator, and batches of 32 to 1 100 proofs that reach every scan width."""
import functools

import numpy as np
import pytest

from tests import interaction_ref as R
from tests import oracle_binding as ob
from tests.chain_harness import chain, eval_column, full, inputs_of, lookup_of, oods_of, pin_id, pins, u32, walks_of, weights
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
P = R.P


def _balance(sums, inputs, z, alpha):
    t = R.q_add(R.q_add(R.q(sums[0]), R.q(sums[1])), R.q(R.input_sum(inputs, z, alpha)))
    return not t.any()


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_tree2_is_what_the_next_fixture_proves(rsv, pin):
    """The library alone: program -> witness_interaction with K+1's (z, alpha) -> K+1's claimed sums, its 24 tree-2 sampled
    values, and the balance identity with the circuit's public inputs."""
    from oracle import recursion_circuit as rc
    src, mult, dst = pin["src"], pin["multiplier"], pin["dst"]
    wp = rsv.WitnessProgram.build(read_proof(src), fixture_cfg(src), inputs_of(src), copies=mult, set_walks=walks_of(pin))
    z, alpha = lookup_of(dst)
    ip, iq, sums, ok, accept, _ = rsv.witness_interaction([read_proof(src)], wp, (z, alpha), inputs_of(src))
    assert accept[0] == 1 and ok[0] == 1
    d = rc.parse_proof(read_proof(dst))
    assert tuple(sums[0, 0].tolist()) == tuple(d.plonk_total_sum)
    assert tuple(sums[0, 1].tolist()) == tuple(d.poseidon_total_sum)
    lp, lq = wp.trace_sizes()
    oods = oods_of(dst)
    got = []
    for log, cols in ((lp, ip[0]), (lq, iq[0])):
        w, wprev = weights(log, oods), weights(log, R.prev_row_point(oods, log))
        for k in range(8):
            got.append([eval_column(w, cols[k])] if k < 4 else [eval_column(wprev, cols[k]), eval_column(w, cols[k])])
    want = [[tuple(v) for v in col] for col in d.sampled_values[2]]
    assert got == want, [k for k in range(16) if got[k] != want[k]]
    assert _balance(sums[0].tolist(), inputs_of(dst), z, alpha)
    wp.close()


def _expected(rsv, wp, plonk, poseidon, z, alpha):
    """The restatement from one proof's GPU trace columns -> (int_plonk, int_poseidon, sums [2][4], ok)."""
    ppre, qpre = wp.preprocessed()
    lp, lq = wp.trace_sizes()
    cp, cq, sums, ok = R.interaction(ppre.astype(np.int64), plonk.astype(np.int64), qpre.astype(np.int64), poseidon.astype(np.int64),
                                     z, alpha, lp, lq)
    return cp.astype(np.uint32), cq.astype(np.uint32), np.array(sums, np.uint32), ok


def _device(rsv, ctx, wp, batch, inputs, lookup, layout):
    """The chain through Context.witness_trace, then Context.witness_interaction on tensors in HBM (outputs prefilled: every
    element must be written) -> numpy int_plonk, int_poseidon, sums, ok, accept, plonk trace, poseidon trace."""
    import torch
    n = len(batch)
    ctx.set_option("witness_layout", layout)
    ch = chain(rsv, ctx, wp, batch, inputs, 1, upto="trace", by_variable=layout == "by_variable")
    lp, lq = wp.trace_sizes()
    d_lookup = torch.from_numpy(rsv._lookup_array(lookup, n).view(np.int32)).to(ch.device)
    d_ip, d_iq, d_sums = full((n, 8, 1 << lp)), full((n, 8, 1 << lq)), full((n, 2, 4))
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device=ch.device)
    ctx.witness_interaction(wp, ch.plonk, ch.poseidon, ch.acc, d_lookup, n, d_ip, d_iq, d_sums, d_ok)
    got = ch.numpy()
    ctx.set_option("witness_layout", "by_proof")
    return u32(d_ip), u32(d_iq), u32(d_sums), d_ok.cpu().numpy(), got["acc"], got["plonk"], got["poseidon"]


def _random_lookup(rng, n):
    return [(tuple(int(x) for x in rng.integers(0, P, 4)), tuple(int(x) for x in rng.integers(0, P, 4))) for _ in range(n)]


def test_mixed_batch_bit_for_bit(rsv):
    """37 proofs of the level10 shape (level10-1 and level11-1), per-proof random (z, alpha), every 17th proof tampered
    (rejected: zero columns, zero sums, ok = 0): every accepted proof equals the restatement on its own GPU trace columns and
    balances the public inputs; both variable layouts on the device equal the host form."""
    wp = rsv.WitnessProgram.build(read_proof("level10-1.bin"), fixture_cfg("level10-1.bin"))
    names = ["level10-1.bin" if k % 3 == 0 else "level11-1.bin" for k in range(37)]
    batch = [ob.tamper(read_proof(nm), 11) if k % 17 == 0 else read_proof(nm) for k, nm in enumerate(names)]
    rng = np.random.default_rng(2024)
    lookup = _random_lookup(rng, 37)
    ip, iq, sums, ok, accept, reason = rsv.witness_interaction(batch, wp, lookup)
    rejected = [k for k in range(37) if k % 17 == 0]
    assert accept.tolist() == [0 if k in rejected else 1 for k in range(37)]
    assert ok.tolist() == accept.tolist()
    plonk, poseidon, _, acc2, _ = rsv.witness_trace([read_proof("level10-1.bin"), read_proof("level11-1.bin")], wp)
    assert acc2.tolist() == [1, 1]
    trace = {"level10-1.bin": (plonk[0], poseidon[0]), "level11-1.bin": (plonk[1], poseidon[1])}
    inputs = inputs_of("level11-1.bin")
    for k, nm in enumerate(names):
        if k in rejected:
            assert not ip[k].any() and not iq[k].any() and not sums[k].any(), k
            continue
        wpl, wpo, wsums, wok = _expected(rsv, wp, *trace[nm], *lookup[k])
        assert wok
        assert np.array_equal(ip[k], wpl), k
        assert np.array_equal(iq[k], wpo), k
        assert np.array_equal(sums[k], wsums), k
        assert _balance(sums[k].tolist(), inputs, *lookup[k]), k
    ctx = rsv.Context(0)
    for layout in ("by_proof", "by_variable"):
        dp, dq, ds, dok, da, _, _ = _device(rsv, ctx, wp, batch, rsv.STANDARD_INPUTS, lookup, layout)
        assert np.array_equal(da, accept) and np.array_equal(dok, ok), layout
        assert np.array_equal(dp, ip) and np.array_equal(dq, iq) and np.array_equal(ds, sums), layout
    ctx.close()
    wp.close()


def test_one_proof_device_call_and_zero_denominator(rsv):
    """A 1-proof device call equals the host form; then a batch of five in which proof 2's z is crafted so that one Plonk
    row's denominator is zero: that proof gets ok = 0 and zero output, its neighbours are bit-identical to a clean run."""
    wp = rsv.WitnessProgram.build(read_proof("level10-1.bin"), fixture_cfg("level10-1.bin"))
    proof = read_proof("level10-1.bin")
    rng = np.random.default_rng(5)
    ctx = rsv.Context(0)
    lk1 = _random_lookup(rng, 1)
    dp, dq, ds, dok, da, plonk, _ = _device(rsv, ctx, wp, [proof], rsv.STANDARD_INPUTS, lk1, "by_proof")
    hp, hq, hs, hok, ha, _ = rsv.witness_interaction([proof], wp, lk1)
    assert da[0] == 1 and dok[0] == 1 and hok[0] == 1
    assert np.array_equal(dp, hp) and np.array_equal(dq, hq) and np.array_equal(ds, hs)
    # z = a_val + alpha a_wire at row 3: the a-entry's denominator of that row is zero
    lookup = _random_lookup(rng, 5)
    alpha = lookup[2][1]
    ppre, _ = wp.preprocessed()
    row = 3
    a_val = R.q(plonk[0][0:4, row])
    z = R.q_add(a_val, R.q_mul_m(R.q(alpha), int(ppre[0][row])))
    lookup[2] = (tuple(int(x) for x in z[:, 0]), alpha)
    batch = [proof] * 5
    dp, dq, ds, dok, da, _, _ = _device(rsv, ctx, wp, batch, rsv.STANDARD_INPUTS, lookup, "by_proof")
    assert da.tolist() == [1] * 5 and dok.tolist() == [1, 1, 0, 1, 1]
    assert not dp[2].any() and not dq[2].any() and not ds[2].any()
    clean = list(lookup)
    clean[2] = lookup[0]
    cp, cq, cs, cok, _, _, _ = _device(rsv, ctx, wp, batch, rsv.STANDARD_INPUTS, clean, "by_proof")
    assert cok.tolist() == [1] * 5
    for k in (0, 1, 3, 4):
        assert np.array_equal(dp[k], cp[k]) and np.array_equal(dq[k], cq[k]) and np.array_equal(ds[k], cs[k]), k
    # the restatement agrees that proof 2 has a zero denominator
    _, _, _, wok = _expected(rsv, wp, plonk[0], _device_trace_poseidon(rsv, wp, proof), *lookup[2])
    assert not wok
    ctx.close()
    wp.close()


def _device_trace_poseidon(rsv, wp, proof):
    _, poseidon, _, acc, _ = rsv.witness_trace([proof], wp)
    assert acc[0] == 1
    return poseidon[0]


def test_five_copies_batch(rsv):
    """A copies = 5 program (2^19 Plonk, 2^18 Poseidon rows): a device batch with a rejected proof equals the restatement on
    its own trace columns for the accepted ones, and zero for the rejected one."""
    pin = next(p for p in pins() if p["multiplier"] == 5 and p["src"] == "recursive_proof_16_15.bin")
    src = pin["src"]
    wp = rsv.WitnessProgram.build(read_proof(src), fixture_cfg(src), inputs_of(src), copies=5, set_walks=walks_of(pin))
    assert wp.trace_sizes() == (19, 18)
    batch = [read_proof(src), ob.tamper(read_proof(src), 3), read_proof(src)]
    rng = np.random.default_rng(11)
    lookup = _random_lookup(rng, 3)
    ctx = rsv.Context(0)
    dp, dq, ds, dok, da, plonk, poseidon = _device(rsv, ctx, wp, batch, inputs_of(src), lookup, "by_proof")
    assert da.tolist() == [1, 0, 1] and dok.tolist() == [1, 0, 1]
    assert not dp[1].any() and not dq[1].any() and not ds[1].any()
    for k in (0, 2):
        wpl, wpo, wsums, wok = _expected(rsv, wp, plonk[k], poseidon[k], *lookup[k])
        assert wok and np.array_equal(dp[k], wpl) and np.array_equal(dq[k], wpo) and np.array_equal(ds[k], wsums), k
        assert _balance(ds[k].tolist(), inputs_of(pin["dst"]), *lookup[k])
    ctx.close()
    wp.close()


def test_api_errors(rsv):
    """NULL inputs, a program without a gate list."""
    import torch
    dev = torch.device("cuda:0")
    wp = rsv.WitnessProgram.build(read_proof("level10-1.bin"), fixture_cfg("level10-1.bin"))
    lp, lq = wp.trace_sizes()
    ctx = rsv.Context(0)
    d_acc = torch.ones(1, dtype=torch.uint8, device=dev)
    d_plonk = torch.zeros((1, 12, 1 << lp), dtype=torch.int32, device=dev)
    d_pos = torch.zeros((1, 48, 1 << lq), dtype=torch.int32, device=dev)
    d_lk = torch.zeros((1, 8), dtype=torch.int32, device=dev)
    d_ip = torch.zeros((1, 8, 1 << lp), dtype=torch.int32, device=dev)
    d_iq = torch.zeros((1, 8, 1 << lq), dtype=torch.int32, device=dev)
    d_sums = torch.zeros((1, 2, 4), dtype=torch.int32, device=dev)
    with pytest.raises(rsv.RsvError) as e:
        ctx.witness_interaction(wp, None, d_pos, d_acc, d_lk, 1, d_ip, d_iq, d_sums)
    assert e.value.code == -1
    with pytest.raises(rsv.RsvError) as e:
        ctx.witness_interaction(wp, d_plonk, d_pos, d_acc, d_lk, 1, d_ip, d_iq, None)
    assert e.value.code == -1
    loaded = rsv.WitnessProgram(wp.export())
    with pytest.raises(rsv.RsvError) as e:
        ctx.witness_interaction(loaded, d_plonk, d_pos, d_acc, d_lk, 1, d_ip, d_iq, d_sums)
    assert e.value.code == -2
    with pytest.raises(rsv.RsvError) as e:
        rsv.witness_interaction([read_proof("level10-1.bin")], loaded, ((0,) * 4, (0,) * 4))
    assert e.value.code == -2
    loaded.close()
    ctx.close()
    wp.close()


def test_alignment_and_batch_limit(rsv):
    """RSV_E_SIZE, with nothing written, for a misaligned input or output (4 bytes for the trace columns, the lookup elements
    and the sums, 8 for the interaction columns) and for a batch beyond 2^20 proofs."""
    import torch
    dev = torch.device("cuda:0")
    wp = rsv.WitnessProgram.build(read_proof("level10-1.bin"), fixture_cfg("level10-1.bin"))
    lp, lq = wp.trace_sizes()
    ctx = rsv.Context(0)
    u8 = lambda words: torch.zeros(4 * words + 8, dtype=torch.uint8, device=dev)
    d_acc = torch.ones(1, dtype=torch.uint8, device=dev)
    ok = {"plonk": u8(12 << lp)[:-8], "poseidon": u8(48 << lq)[:-8], "lookup": u8(8)[:-8], "ip": u8((8 << lp) + 2)[:-8],
          "iq": u8((8 << lq) + 2)[:-8], "sums": u8(8)[:-8]}
    shifted = {"plonk": u8(12 << lp)[1:-7], "poseidon": u8(48 << lq)[2:-6], "lookup": u8(8)[3:-5], "ip": u8((8 << lp) + 2)[4:-4],
               "iq": u8((8 << lq) + 2)[4:-4], "sums": u8(8)[1:-7]}
    for k in ok:
        args = dict(ok, **{k: shifted[k]})
        for t in (args["ip"], args["iq"], args["sums"]):
            t.fill_(0x5A)
        with pytest.raises(rsv.RsvError) as e:
            ctx.witness_interaction(wp, args["plonk"], args["poseidon"], d_acc, args["lookup"], 1, args["ip"], args["iq"], args["sums"])
        assert e.value.code == -2, k
        ctx.synchronize()
        assert all(bool((t == 0x5A).all()) for t in (args["ip"], args["iq"], args["sums"])), k
    with pytest.raises(rsv.RsvError) as e:
        ctx.witness_interaction(wp, ok["plonk"], ok["poseidon"], d_acc, ok["lookup"], (1 << 20) + 1, ok["ip"], ok["iq"], ok["sums"])
    assert e.value.code == -2
    # the aligned call on the same buffers goes through
    ctx.witness_interaction(wp, ok["plonk"], ok["poseidon"], d_acc, ok["lookup"], 1, ok["ip"], ok["iq"], ok["sums"])
    ctx.synchronize()
    ctx.close()
    wp.close()


# (n, B): B = clamp(17 - min(ceil(log2 n), 10), 7, 12), then B <= log - 1 (interaction_chunk_bits, interaction_api.inc), the
# same for both components of the level10 shape (2^16 and 2^15 rows)
SWEEP = [(32, 12), (33, 11), (65, 10), (129, 9), (257, 8), (513, 7), (1100, 7)]
N_POOL = 6


def _scan_bits(n, log):
    return min(max(17 - min((n - 1).bit_length(), 10), 7), 12, log - 1)


@functools.lru_cache(maxsize=None)
def _sweep_pool(rsv):
    """The device trace columns of level10-1 and level11-1 under the level10 program, a pool of N_POOL random (z, alpha), a
    lookup crafted for a zero denominator in a late Plonk row of level10-1, and the restatement of every (trace, lookup)
    pair: (plonk [2, 12, 2^lp], poseidon [2, 48, 2^lq], lookup words [N_POOL + 1, 8], expected int_plonk / int_poseidon /
    sums with an all-zero entry last)."""
    wp = rsv.WitnessProgram.build(read_proof("level10-1.bin"), fixture_cfg("level10-1.bin"))
    plonk, poseidon, _, acc, _ = rsv.witness_trace([read_proof("level10-1.bin"), read_proof("level11-1.bin")], wp)
    assert acc.tolist() == [1, 1]
    lp, lq = wp.trace_sizes()
    rng = np.random.default_rng(1100)
    pool = _random_lookup(rng, N_POOL + 1)
    ppre, _ = wp.preprocessed()
    row = (1 << lp) - 5
    alpha = pool[N_POOL][1]
    z = R.q_add(R.q(plonk[0][0:4, row]), R.q_mul_m(R.q(alpha), int(ppre[0][row])))
    pool[N_POOL] = (tuple(int(x) for x in z[:, 0]), alpha)
    ep = np.zeros((2 * N_POOL + 1, 8, 1 << lp), np.uint32)
    eq = np.zeros((2 * N_POOL + 1, 8, 1 << lq), np.uint32)
    es = np.zeros((2 * N_POOL + 1, 2, 4), np.uint32)
    for s in range(2):
        for j in range(N_POOL):
            ep[N_POOL * s + j], eq[N_POOL * s + j], es[N_POOL * s + j], wok = _expected(rsv, wp, plonk[s], poseidon[s], *pool[j])
            assert wok, (s, j)
    assert not _expected(rsv, wp, plonk[0], poseidon[0], *pool[N_POOL])[3]
    words = rsv._lookup_array(pool, N_POOL + 1)
    wp.close()
    return plonk, poseidon, words, ep, eq, es


@pytest.mark.parametrize("n,B", SWEEP, ids=[f"n{n}-B{B}" for n, B in SWEEP])
def test_every_scan_width(rsv, n, B):
    """n proofs of the level10 shape in one rsv_witness_interaction_dev call, so that the scan width is B =
    clamp(17 - min(ceil(log2 n), 10), 7, 12) (interaction_chunk_bits): 12, 11, 10, 9, 8, 7, 7 for n = 32, 33, 65, 129, 257,
    513, 1100 — the chunk boundaries, the cc << (log - B) shift terms of k_int_offsets (at B = 7, 128 of its 4 096 slots,
    all in wave 0) and the backward walk of k_int_scan.  Each proof takes level10-1's or level11-1's device trace columns and
    one (z, alpha) of a pool; proofs 3 and n - 1 (and 70, 200, 700 where n allows) have accept = 0, proofs n / 2 + 1 and
    n - 2 a zero denominator.  Every proof's columns equal the restatement, compared on the device; sums and ok too; the
    rejected and zero-denominator proofs are all zeros with ok = 0."""
    import torch
    dev = torch.device("cuda:0")
    assert _scan_bits(n, 16) == _scan_bits(n, 15) == B
    plonk, poseidon, words, ep, eq, es = _sweep_pool(rsv)
    wp = rsv.WitnessProgram.build(read_proof("level10-1.bin"), fixture_cfg("level10-1.bin"))
    lp, lq = wp.trace_sizes()
    rng = np.random.default_rng(n)
    src = rng.integers(0, 2, n)
    lk = rng.integers(0, N_POOL, n)
    rejected = {3, n - 1} | {k for k in (70, 200, 700) if k < n - 1}
    zero_den = {n // 2 + 1, n - 2}
    assert not rejected & zero_den
    for k in zero_den:
        src[k], lk[k] = 0, N_POOL
    accept = np.array([0 if k in rejected else 1 for k in range(n)], np.uint8)
    want = np.where(accept == 1, N_POOL * src + lk, 2 * N_POOL)
    want[sorted(zero_den)] = 2 * N_POOL
    d_src = torch.from_numpy(src).to(dev)
    d_plonk = torch.from_numpy(plonk.view(np.int32)).to(dev).index_select(0, d_src)
    d_pos = torch.from_numpy(poseidon.view(np.int32)).to(dev).index_select(0, d_src)
    d_acc = torch.from_numpy(accept).to(dev)
    d_lookup = torch.from_numpy(words[lk].view(np.int32)).to(dev)
    d_ip = torch.full((n, 8, 1 << lp), -1, dtype=torch.int32, device=dev)
    d_iq = torch.full((n, 8, 1 << lq), -1, dtype=torch.int32, device=dev)
    d_sums = torch.full((n, 2, 4), -1, dtype=torch.int32, device=dev)
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ctx = rsv.Context(0)
    ctx.witness_interaction(wp, d_plonk, d_pos, d_acc, d_lookup, n, d_ip, d_iq, d_sums, d_ok)
    ctx.synchronize()
    ctx.close()
    wp.close()
    e_p, e_q = torch.from_numpy(ep.view(np.int32)).to(dev), torch.from_numpy(eq.view(np.int32)).to(dev)
    d_want = torch.from_numpy(want).to(dev)
    wrong = []
    for k0 in range(0, n, 64):
        k1 = min(n, k0 + 64)
        same = (d_ip[k0:k1] == e_p.index_select(0, d_want[k0:k1])).flatten(1).all(1)
        same &= (d_iq[k0:k1] == e_q.index_select(0, d_want[k0:k1])).flatten(1).all(1)
        wrong += [k0 + int(i) for i in torch.nonzero(~same).flatten().tolist()]
    assert not wrong, wrong[:16]
    assert np.array_equal(d_sums.cpu().numpy().view(np.uint32), es[want])
    assert d_ok.cpu().numpy().tolist() == [0 if k in rejected | zero_den else 1 for k in range(n)]
    del d_plonk, d_pos, d_ip, d_iq
    torch.cuda.empty_cache()
