"""rsv_witness_trace / rsv_witness_trace_dev (`-m gpu`): the 110 columns the next prover commits for the recursion circuit.
Against the REFERENCE for all 14 consecutive fixture pairs (every column, interpolated at fixture K+1's OODS point, is the
sampled value K+1 carries), and bit for bit, on a mixed batch, against the oracle's restatement of
generate_plonk_with_poseidon_circuit (oracle/recursion_circuit/trace.py) fed with the GPU's own variables and flow (which
tests/test_witness_gpu.py pins to the oracle's gadgets)."""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests.chain_harness import chain, eval_column, inputs_of, pin_id, pins, round_constants, walks_of, weights
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_all_110_columns_are_what_the_next_fixture_proves(rsv, pin):
    """The library alone — program, preprocessed columns (op patched with the proof's d_ops), trace columns from the GPU —
    gives every one of the next fixture's 50 preprocessed and 60 trace sampled values."""
    from oracle import recursion_circuit as rc
    src, mult = pin["src"], pin["multiplier"]
    wp = rsv.WitnessProgram.build(read_proof(src), fixture_cfg(src), inputs_of(src), copies=mult, set_walks=walks_of(pin))
    plonk, poseidon, ops, accept, _ = rsv.witness_trace([read_proof(src)], wp, inputs_of(src))
    assert accept[0] == 1
    ppre, qpre = wp.preprocessed()
    _, wops = wp.gates()
    ppre[3, wops[:, 0]] = ops[0]
    nxt = read_proof(pin["dst"])
    lp, lq = (int(x) for x in np.frombuffer(nxt[:8], np.uint32))
    assert wp.trace_sizes() == (lp, lq) and plonk.shape[2] == 1 << lp and poseidon.shape[2] == 1 << lq
    tr = ob.transcript_raw(nxt)
    oods = (tuple(int(x) for x in tr[20:24]), tuple(int(x) for x in tr[24:28]))
    want = rc.parse_proof(nxt).sampled_values
    wp_, wq = weights(lp, oods), weights(lq, oods)
    pre_cols = [(wp_, c) for c in ppre] + [(wq, c) for c in qpre]
    tr_cols = [(wp_, c) for c in plonk[0]] + [(wq, c) for c in poseidon[0]]
    assert len(pre_cols) == 50 and len(tr_cols) == 60
    bad = [k for k, (w, c) in enumerate(pre_cols) if eval_column(w, c) != tuple(want[0][k][0])]
    bad += [50 + k for k, (w, c) in enumerate(tr_cols) if eval_column(w, c) != tuple(want[1][k][0])]
    assert not bad, bad
    wp.close()


def _expected(rsv, wp, variables, flow, swap):
    """The oracle's trace columns from one proof's GPU variables and flow: int64[12, 2^lp], int64[48, 2^lq], ops."""
    from oracle import recursion_circuit as rc
    from oracle.recursion_circuit import trace as T
    lp, lq = wp.trace_sizes()
    rows, wops = wp.gates(variables)
    wires = wp.export().flow_wires
    mult = wp.shape.copies
    c = rc.cs.ConstraintSystem()
    c.variables = [tuple(int(x) for x in v) for v in variables]
    c.a_wire, c.b_wire, c.c_wire, c.op, c.poseidon_wire, c.enforce_c_m31 = (rows[:, k].tolist() for k in range(6))
    c.flow = []
    assert T.pad(c) == 1 << lp
    _, plonk = T.plonk_columns(c)
    recs = [((int(w[0]), tuple(int(x) for x in f[0:8])), (int(w[1]), tuple(int(x) for x in f[8:16])), (int(w[2]), tuple(int(x) for x in f[16:24])),
             (int(w[3]), tuple(int(x) for x in f[24:32])), int(w[4]), bool(sw))
            for w, f, sw in zip(wires, np.tile(flow, (mult, 1)), np.tile(swap, mult))]
    n_pad = max(32, -(-len(recs) // 16) * 16)
    for _ in range(len(recs), n_pad):
        recs.append(((0, None), (0, None), (0, None), (0, None), 0, False))
    _, poseidon = T.poseidon_columns(recs, round_constants(), lq, padding_hash=([0] * 8,))
    ops = np.where(variables[wops[:, 1], 0] != 0, wops[:, 2], 0).astype(np.uint32)
    return plonk.astype(np.int64), poseidon.astype(np.int64), ops, n_pad


def _device_trace(rsv, ctx, wp, batch, inputs, layout, plonk=True, poseidon=True, ops=True):
    """The chain through Context.witness_trace on tensors in HBM under a variable layout (outputs prefilled: every element
    must be written) -> numpy plonk, poseidon, ops, accept (None for a skipped output)."""
    ctx.set_option("witness_layout", layout)
    got = chain(rsv, ctx, wp, batch, inputs, 1, upto="trace", by_variable=layout == "by_variable",
                outputs={"plonk": plonk, "poseidon": poseidon, "ops": ops}).numpy()
    ctx.set_option("witness_layout", "by_proof")
    return got.get("plonk"), got.get("poseidon"), got.get("ops"), got["acc"]


def test_mixed_batch_bit_for_bit(rsv):
    """37 proofs of the level10 shape (level10-1 as the template, level11-1, one of them bit-flipped): accepted rows equal the
    oracle's columns of that proof, rejected rows and ops are zero, the Poseidon rows behind the padded flow are zero; the
    device path under both variable layouts, and the Plonk-only / Poseidon-only calls, equal the host path."""
    import torch
    wp = rsv.WitnessProgram.build(read_proof("level10-1.bin"), fixture_cfg("level10-1.bin"))
    names = ["level10-1.bin" if k % 3 == 0 else "level11-1.bin" for k in range(37)]
    batch = [read_proof(nm) for nm in names]
    batch[13] = ob.tamper(read_proof(names[13]), 11)
    plonk, poseidon, ops, accept, reason = rsv.witness_trace(batch, wp)
    assert accept.tolist() == [0 if k == 13 else 1 for k in range(37)] and reason[13] != 0
    variables, acc2, _, flow, swap = rsv.witness([read_proof("level10-1.bin"), read_proof("level11-1.bin")], wp, with_flow=True)
    assert acc2.tolist() == [1, 1]
    want = {nm: _expected(rsv, wp, variables[i], flow[i], swap[i]) for i, nm in enumerate(["level10-1.bin", "level11-1.bin"])}
    assert not np.array_equal(want["level10-1.bin"][0], want["level11-1.bin"][0])
    assert not np.array_equal(want["level10-1.bin"][1], want["level11-1.bin"][1])
    for k, nm in enumerate(names):
        if k == 13:
            assert not plonk[k].any() and not poseidon[k].any() and not ops[k].any()
            continue
        wpl, wpo, wops, n_pad = want[nm]
        assert np.array_equal(plonk[k], wpl), k
        assert np.array_equal(poseidon[k], wpo), k
        assert not poseidon[k][:, 6 * n_pad:].any()
        assert np.array_equal(ops[k], wops), k
    ctx = rsv.Context(0)
    for layout in ("by_proof", "by_variable"):
        dp, dq, do, da = _device_trace(rsv, ctx, wp, batch, rsv.STANDARD_INPUTS, layout)
        assert np.array_equal(da, accept) and np.array_equal(dp, plonk) and np.array_equal(dq, poseidon) and np.array_equal(do, ops), layout
    dp, dq, do, _ = _device_trace(rsv, ctx, wp, batch, rsv.STANDARD_INPUTS, "by_variable", poseidon=False, ops=False)
    assert dq is None and do is None and np.array_equal(dp, plonk)
    dp, dq, do, _ = _device_trace(rsv, ctx, wp, batch, rsv.STANDARD_INPUTS, "by_proof", plonk=False)
    assert dp is None and np.array_equal(dq, poseidon) and np.array_equal(do, ops)
    # API errors: NULL variables with a Plonk output, a program without a gate list
    dev = torch.device("cuda:0")
    lp, _ = wp.trace_sizes()
    d_acc = torch.ones(1, dtype=torch.uint8, device=dev)
    d_plonk = torch.zeros((1, 12, 1 << lp), dtype=torch.int32, device=dev)
    with pytest.raises(rsv.RsvError) as e:
        ctx.witness_trace(wp, None, d_acc, 1, d_plonk=d_plonk)
    assert e.value.code == -1
    loaded = rsv.WitnessProgram(wp.export())
    d_vars = torch.zeros((1, loaded.n_vars, 4), dtype=torch.int32, device=dev)
    with pytest.raises(rsv.RsvError) as e:
        ctx.witness_trace(loaded, d_vars, d_acc, 1, d_plonk=d_plonk)
    assert e.value.code == -2
    with pytest.raises(rsv.RsvError) as e:
        rsv.witness_trace([read_proof("level10-1.bin")], loaded)
    assert e.value.code == -2
    assert rsv.lib.rsv_witness_trace(loaded._h, None, None, 0, None, None, 0, None, None, None, None, None, 0) == -2
    loaded.close()
    ctx.close()
    wp.close()


def test_five_copies_batch(rsv):
    """A copies = 5 program (examples/multi-proofs' circuit: 2^19 Plonk, 2^18 Poseidon rows): a batch with a rejected proof
    on the device equals the single-proof host call row for row (that call is pinned to the next fixture above), and the
    five copies' Poseidon blocks hash the same records."""
    pin = next(p for p in pins() if p["multiplier"] == 5 and p["src"] == "recursive_proof_16_15.bin")
    src = pin["src"]
    wp = rsv.WitnessProgram.build(read_proof(src), fixture_cfg(src), inputs_of(src), copies=5, set_walks=walks_of(pin))
    plonk1, poseidon1, ops1, acc1, _ = rsv.witness_trace([read_proof(src)], wp, inputs_of(src))
    assert acc1[0] == 1 and wp.trace_sizes() == (19, 18)
    batch = [read_proof(src), ob.tamper(read_proof(src), 3), read_proof(src)]
    ctx = rsv.Context(0)
    dp, dq, do, da = _device_trace(rsv, ctx, wp, batch, inputs_of(src), "by_proof")
    assert da.tolist() == [1, 0, 1]
    for k in (0, 2):
        assert np.array_equal(dp[k], plonk1[0]) and np.array_equal(dq[k], poseidon1[0]) and np.array_equal(do[k], ops1[0])
    assert not dp[1].any() and not dq[1].any() and not do[1].any()
    # invocation k of copy c hashes record k - c * flow_count: the in[] words of row 0 repeat per copy
    F = wp.shape.flow_count
    rows0 = lambda k: ((k // 16) * 6) * 16 + k % 16
    for k in (0, 1, 17, F - 1):
        for c in range(1, 5):
            assert np.array_equal(poseidon1[0][:16, rows0(k)], poseidon1[0][:16, rows0(c * F + k)])
    ctx.close()
    wp.close()
