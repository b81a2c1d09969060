"""No result depends on what a workspace held before the call (`-m gpu`).

The library never initialises its device scratch: every context workspace is a bare allocation that each call carves again
at its own shape (csrc/verify_api.inc: ensure_buf), and correctness rests on presets and written-before-read orders that
DESIGN.md lists ("Workspaces: who writes first").  Two things make a mistake in them visible here.

1. RSV_OPT_WS_FILL ("ws_fill" = 1 + byte, set as the process default BEFORE the context exists): every byte of the library's
   own scratch holds the byte before a call's first kernel can touch it.  Three bytes, each hiding a different mistake:
   0x00 shows a missing all-ones preset (a missing zeroing does not show), 0xFF the reverse (words >= P, and the "nothing
   found" value of the atomicMin cells), 0x5A a plausible canonical field word (0x5A5A5A5A < P).  Caller-owned scratch and
   every output is filled by the test with the same byte.
2. The knob off, ONE context, a different call in between: call A (shape X, mask m1), call B (a larger shape, every proof
   accepted, another n), call A' (shape X again, fewer proofs, another mask).  That is real stale content, and it finds a
   cache keyed by too little, which a fill cannot.

Every comparison is with the reference — the C oracle (tests/oracle_binding.py), a fixture's file, or the numpy restatements
(tests/*_ref.py) — exact on every word; a comparison with the unfilled run stands beside it where the issue is bytes."""
import numpy as np
import pytest

from tests import circuit_eval_ref as E
from tests import commit_ref as C
from tests import composition_ref as K
from tests import decommit_ref as D
from tests import fri_open_ref as FO
from tests import fri_ref as F
from tests import oracle_binding as ob
from tests import pack_ref as PR
from tests import pow_ref as W
from tests import sample_ref as S
from tests import statement_ref as ST
from tests import user_circuit_ref as U
from tests import witness_inputs_ref as WI
from tests.chain_harness import CASES, DEV, FILL, chain, dev, inputs_of, mask_dev, pin_of, program_of, tail, u32
from tests.conftest import fixture_cfg, load_manifest, read_proof

pytestmark = pytest.mark.gpu
P = C.P
BYTES = [0x00, 0xFF, 0x5A]
byte_id = "fill{:02x}".format
NONE = U.NONE
S1_CONFIG = (3, 1, 0, 9)   # (pow_bits, log_blowup, log_last, n_queries): tests/test_user_circuit_gpu.py's first


def _filled(byte, shape, dtype=None):
    """A device tensor whose every BYTE is the fill byte: what the tests leave in outputs and in caller-owned scratch."""
    import torch
    dtype = dtype or torch.int32
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(byte)
    return t


def _context(rsv, knobs, byte):
    """A context born under the fill (byte None: the knob off)."""
    knobs.set("ws_fill", 0 if byte is None else byte + 1)
    return rsv.Context(0)


def _to_dev(proofs, rsv):
    import torch
    blob, offsets = rsv.pack(proofs)
    return torch.from_numpy(blob.copy()).to(DEV), torch.from_numpy(offsets.astype(np.int64)).to(DEV)


def _verify_ctx(rsv, ctx, proofs, cfg, byte=0x07, **kw):
    import torch
    n = len(proofs)
    d_blob, d_off = _to_dev(proofs, rsv)
    d_acc, d_reason = _filled(byte, (n,), torch.uint8), _filled(byte, (n,), torch.uint8)
    ctx.verify_batch(d_blob, d_off, n, d_acc, d_reason, cfg=cfg, **kw)
    ctx.synchronize()
    return d_acc.cpu().numpy().tolist(), d_reason.cpu().numpy().tolist()


# ---------------------------------------------------------------- verify: ws, ws_fixed, ws_rows, d_pi
_MIXED = {}


def _mixed_batch():
    """The 15 accepted fixtures, a tampered copy of each, a garbage proof and an empty one, each under its own
    configuration, and the oracle's verdicts and reasons under the three standard inputs (small_proof.bin, whose circuit has
    one input, is rejected by both)."""
    if not _MIXED:
        names = [e["file"] for e in load_manifest() if e["expect"] == "ok"]
        assert len(names) == 15
        rng = np.random.default_rng(77)
        proofs, cfgs = [], []
        for k, nm in enumerate(names):
            proofs += [read_proof(nm), ob.tamper(read_proof(nm), 31 * k + 5)]
            cfgs += [fixture_cfg(nm)] * 2
        proofs += [rng.integers(0, 256, 4096, dtype=np.uint8).tobytes(), b""]
        cfgs += [fixture_cfg(names[0]), fixture_cfg(names[1])]
        acc, reason = ob.verify_batch(proofs, cfgs)
        assert acc[::2][1:15].tolist() == [1] * 14 and not acc[-2:].any()
        _MIXED.update(proofs=proofs, cfgs=cfgs, acc=acc.tolist(), reason=reason.tolist())
    return _MIXED


FORMS = {"default": {}, "tree_pace=row16": {"tree_pace": "row16"}, "tree_pace=paced": {"tree_pace": "paced"},
         "query_form=lane": {"query_form": "lane"}, "cap_top=on,cap_mid=on": {"cap_top": "on", "cap_mid": "on"},
         "plan_form=serial": {"plan_form": "serial"}, "ws_budget_mb=1": {"ws_budget_mb": 1}}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_verify_mixed_batch(rsv, knobs, byte, form):
    """rsv_verify_batch on the mixed batch, by default and under every forced form (ws_budget_mb = 1: several launch groups
    that share the per-query workspace): verdict and reason are the oracle's.  The host-pointer call allocates its own
    buffers (DevBuf) and its own context; both inherit the fill."""
    m = _mixed_batch()
    knobs.set("ws_fill", byte + 1)
    for name, value in FORMS[form].items():
        knobs.set(name, value)
    acc, reason = rsv.verify_batch(m["proofs"], m["cfgs"])
    assert acc.tolist() == m["acc"] and reason.tolist() == m["reason"]


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_verify_hints_outputs(rsv, knobs, byte):
    """rsv_verify_hints_dev on small_proof.bin x 3, the middle one tampered, and a truncated copy: the transcript rows, the trace paths and their
    columns, the FRI paths and first-layer folds, the per-query values, the flow and its counts are the oracle's."""
    import torch
    name = "small_proof.bin"
    proof, cfg, inputs = read_proof(name), fixture_cfg(name), inputs_of(name)
    e = next(e for e in load_manifest() if e["file"] == name)
    lay = ob.proof_layout(proof)
    nq, ni = e["n_queries"], lay["n_inner"]
    M = max(e["log_size_plonk"] + 1, e["log_size_poseidon"] + 2) + e["log_blowup_factor"]
    batch = [proof, ob.tamper(proof, 3), proof, proof[:60]]
    n = 4
    oacc, oreason = ob.verify_batch(batch, cfg, inputs)
    assert oacc.tolist() == [1, 0, 1, 0] and oreason[3] == 1
    cnt = rsv.poseidon_flow_count(e["log_size_plonk"], e["log_size_poseidon"], cfg)
    word = byte * 0x01010101

    def run(fill):
        """Every output starts from the fill byte.  The path outputs have a fixed stride and a tree writes only its own levels
        and columns: there the words past them must still hold the byte afterwards."""
        ctx = _context(rsv, knobs, fill)
        d_blob, d_off = _to_dev(batch, rsv)
        o = {"d_transcript": _filled(byte, (n, rsv.TRANSCRIPT_WORDS)), "d_trace_sib": _filled(byte, (n, 4, nq, M, 8)),
             "d_trace_pos": _filled(byte, (n, 4, nq)), "d_trace_cols": _filled(byte, (n, 4, nq, 64)),
             "d_fri_sib": _filled(byte, (n, 1 + ni, nq, M, 8)), "d_fri_cols": _filled(byte, (n, 1 + ni, nq, 3, 8)),
             "d_fri_folded": _filled(byte, (n, 3, nq, 4)), "d_query_values": _filled(byte, (n, nq, 4 * (8 + ni))),
             "d_flow": _filled(byte, (n, cnt, 32)), "d_flow_swap": _filled(byte, (n, cnt), torch.uint8), "d_flow_count": _filled(byte, (n,))}
        d_acc, d_reason = _filled(byte, (n,), torch.uint8), _filled(byte, (n,), torch.uint8)
        ctx.verify_hints(d_blob, d_off, n, d_acc, d_reason, cfg=cfg, inputs=inputs, shape=(nq, M, ni), **o)
        ctx.synchronize()
        out = {k: (v.cpu().numpy() if v.dtype == torch.uint8 else u32(v)) for k, v in o.items()}
        ctx.close()
        assert d_acc.cpu().numpy().tolist() == oacc.tolist() and d_reason.cpu().numpy().tolist() == oreason.tolist()
        return out

    def written_or_prefill(a, want):
        """Word by word: the oracle's, or — where the oracle's fixed-stride array has nothing, a zero — still the prefill."""
        off = a != want
        return not want[off].any() and (a[off] == word).all()

    unfilled, got = run(None), run(byte)
    # a proof rejected behind the parser keeps what its failing verification computed (rsv.h): a function of the proof alone,
    # the same words whatever the workspaces held
    for key in ("d_query_values", "d_flow", "d_flow_swap", "d_flow_count", "d_transcript", "d_fri_folded"):
        assert np.array_equal(got[key][1], unfilled[key][1]), key
    tsib, tpos, depth = ob.trace_paths(proof, nq, M, inputs)
    fsib, fcols = ob.fri_paths(proof, nq, M, 1 + ni, inputs)
    flow = ob.poseidon_flow(proof, inputs)
    raw = ob.transcript_raw(proof)
    na = int(raw[1])
    for k in (0, 2):
        row = got["d_transcript"][k]
        assert np.array_equal(row[:40], raw[:40]) and np.array_equal(row[40:40 + 4 * na], raw[40:40 + 4 * na])
        assert np.array_equal(row[156:156 + nq], raw[40 + 4 * na:40 + 4 * na + nq])
        assert np.array_equal(got["d_trace_pos"][k], tpos)
        for t in range(4):
            d, cols = int(depth[t]), (50, 60, 16, 8)[t]
            assert np.array_equal(got["d_trace_sib"][k, t][:, :d], tsib[t][:, :d]), (k, t)
            assert (got["d_trace_sib"][k, t][:, d:] == word).all(), (k, t)
            assert np.array_equal(got["d_trace_cols"][k, t][:, :cols], ob.trace_cols(proof, inputs)[t][:, :cols]), (k, t)
            assert (got["d_trace_cols"][k, t][:, cols:] == word).all(), (k, t)
        assert written_or_prefill(got["d_fri_cols"][k], fcols), k
        assert np.array_equal(got["d_fri_cols"][k, 0], fcols[0]) and np.array_equal(got["d_fri_cols"][k, 1:, :, 0], fcols[1:, :, 0]), k
        assert np.array_equal(got["d_fri_folded"][k], ob.fri_folded(proof, inputs))
        assert np.array_equal(got["d_query_values"][k], ob.query_dump(proof, inputs))
        assert int(got["d_flow_count"][k]) == cnt == len(flow)
        assert np.array_equal(got["d_flow"][k], flow[:, :32]) and np.array_equal(got["d_flow_swap"][k], flow[:, 32].astype(np.uint8))
    for k in (0, 2):
        for t in range(1 + ni):   # tree t has M - t levels, M - t - 1 siblings per pair path
            d = M if t == 0 else M - t
            assert np.array_equal(got["d_fri_sib"][k, t][:, :d - 1], fsib[t][:, :d - 1]), (k, t)
            assert (got["d_fri_sib"][k, t][:, d - 1:] == word).all(), (k, t)
    # the proof the parser rejected: its transcript row says so and nothing else, its query values are the library's zeros
    assert got["d_transcript"][3, 0] == 1 and not got["d_transcript"][3, 1:].any() and not got["d_query_values"][3].any()
    assert int(got["d_flow_count"][3]) == 0


_S1 = {}


def _s1_witnesses():
    if not _S1:
        _S1["b"] = [E.build("S1", pub=(11 + 7 * k, 0, 0, 0), seed=1 + k, bit=k % 2) for k in range(3)]
    return _S1["b"]


def _s1_circuit(rsv):
    b = _s1_witnesses()[0]
    return rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, **E.create_args(b))


def _s1_chain(rsv, ctx, circ, inputs, flow_in, fill=FILL):
    """Chain.evaluate -> ... -> fri_open of S1 under S1_CONFIG."""
    cfg = rsv.PcsConfig(*S1_CONFIG)
    ch = rsv.Chain(ctx, circ, len(inputs), cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=fill, caps=True, device=DEV)
    ch.evaluate(inputs, flow_in, check=True)
    ctx.synchronize()
    variables = u32(ch._vars)   # trace() drops them
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch, stage)()
    return tail(ch, cfg), cfg, variables


def _oracle_each(proofs, cfg, inputs_per_proof):
    out = [ob.verify_batch([p], cfg, i) for p, i in zip(proofs, inputs_per_proof)]
    return [int(a[0]) for a, _ in out], [int(r[0]) for _, r in out]


def _s1_inputs(bad=None):
    """The free inputs of the three S1 witnesses; bad: that witness's public input is no M31 (its row fails the check)."""
    builts = _s1_witnesses()
    inputs, flow_in = np.stack([E.inputs_of(b) for b in builts]), np.stack([E.flow_in_of(b) for b in builts])
    if bad is not None:
        h = E.hints_of(builts[bad].cs)
        inputs[bad, int(h[(h[:, 0] == 4) & (h[:, 1] == E.INPUT)][0, 3]), 1] = 5
    return inputs, flow_in


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_whole_chain_of_s1_with_a_rejected_witness(rsv, knobs, byte):
    """S1 at n = 3, the middle witness failing its check, from Chain.evaluate through Chain.pack and Chain.verify: the C
    oracle accepts the two proofs under their own statements, Chain.verify's verdicts (rsv_verify_batch_inputs_dev: d_pi_sum)
    are the oracle's with the empty slot a parse reject, the rejected witness's row is the model's, and the bytes equal the
    unfilled run's."""
    builts = _s1_witnesses()
    inputs, flow_in = _s1_inputs(bad=1)
    runs = {}
    for fill in (None, byte):
        ctx = _context(rsv, knobs, fill)
        circ = _s1_circuit(rsv)
        ch, cfg, variables = _s1_chain(rsv, ctx, circ, inputs, flow_in)
        d_acc, d_reason = ch.verify(cfg)
        a = ch.numpy()
        runs[fill] = (ch.proofs(), d_acc.cpu().tolist(), d_reason.cpu().tolist(), a["acc"].tolist(), a["ok"].tolist(), int(a["bad_row"][1]))
        blob, offsets = ch.pack(exact=True)
        off = offsets.cpu().tolist()
        assert [blob.cpu().numpy()[off[k]:off[k + 1]].tobytes() or None for k in range(3)] == runs[fill][0]
        # three proofs with their own statements through the host-pointer form too
        good = [k for k in range(3) if runs[fill][0][k] is not None]
        acc, reason = rsv.verify_batch([runs[fill][0][k] for k in good], cfg, inputs_per_proof=[builts[k].inputs for k in good])
        assert acc.tolist() == [1, 1] and reason.tolist() == [0, 0]
        ctx.close()
        circ.close()
    proofs, vacc, vreason, acc, ok, bad_row = runs[byte]
    assert acc == [1, 0, 1] and ok == [1, 0, 1] and proofs[1] is None
    assert bad_row == U.model_check(builts[1].gates, builts[1].witness_ops, variables[1]) != NONE
    assert _oracle_each([proofs[0], proofs[2]], cfg, [builts[0].inputs, builts[2].inputs]) == ([1, 1], [0, 0])
    assert vacc == [1, 0, 1] and vreason == [0, 1, 0]
    assert runs[byte] == runs[None]


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_circuit_eval_check_and_flow(rsv, knobs, byte):
    """rsv_circuit_eval_dev (both forms), rsv_circuit_check_dev and rsv_circuit_flow_dev on S1 at n = 3, witness 1 with a
    public input that is no M31: variables, flow and swap of the sound witnesses are the oracle's, and the d_bad cells hold
    the row and the invocation the numpy model of the reference's checks names on the evaluated vector."""
    builts = _s1_witnesses()
    inputs, flow_in = _s1_inputs(bad=1)
    cfg = rsv.PcsConfig(*S1_CONFIG)
    ctx = _context(rsv, knobs, byte)
    circ = _s1_circuit(rsv)
    for form in ("per_level", "walk"):
        ctx.set_option("circuit_eval_form", form)
        ch = rsv.Chain(ctx, circ, 3, cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=byte * 0x01010101, caps=True, device=DEV)
        ch.evaluate(inputs, flow_in, check=True)
        a = ch.numpy()
        variables, flow, swap = u32(ch._vars), u32(ch._flow), ch._swap.cpu().numpy()
        want_row = [U.model_check(b.gates, b.witness_ops, variables[k]) for k, b in enumerate(builts)]
        want_flow = [U.model_flow(b.gates, b.flow_wires, variables[k], flow[k])[0] if want_row[k] == NONE else NONE for k, b in enumerate(builts)]
        assert want_row[0] == want_row[2] == NONE and want_row[1] != NONE and want_flow == [NONE] * 3
        assert a["bad_input"].tolist() == [NONE] * 3 and a["bad_row"].tolist() == want_row and a["bad_flow"].tolist() == want_flow, form
        assert a["acc"].tolist() == [1, 0, 1]
        for k in (0, 2):
            assert np.array_equal(variables[k], builts[k].variables) and np.array_equal(flow[k], builts[k].flow) and np.array_equal(swap[k], builts[k].swap)
    ctx.close()
    circ.close()


# ---------------------------------------------------------------- the host-pointer probes (DevBuf)
@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_host_pointer_probes(rsv, knobs, byte):
    knobs.set("ws_fill", byte + 1)
    rng = np.random.default_rng(900 + byte)
    st = rng.integers(0, P, (65, 16), dtype=np.uint32)
    assert np.array_equal(rsv.poseidon2_permute(st), ob.poseidon2_permute(st))
    l, r, cols = (rng.integers(0, P, (300, w), dtype=np.uint32) for w in (8, 8, 17))
    assert np.array_equal(rsv.hash_node((l, r), cols), ob.hash_node((l, r), cols))
    assert np.array_equal(rsv.hash_node(None, cols), ob.hash_node(None, cols))
    a, b = (rng.integers(0, P, (1000, 4), dtype=np.uint32) for _ in range(2))
    for op in range(10):
        bb = b if op in (0, 1, 2, 4, 6) else None
        assert np.array_equal(rsv.field_op(op, a, bb), ob.field_op(op, a, bb)), op
    coeffs, xs = rng.integers(0, P, (1 << 5, 4), dtype=np.uint32), rng.integers(0, P, 70, dtype=np.uint32)
    assert np.array_equal(rsv.line_eval(coeffs, xs), ob.line_eval(coeffs, xs))
    sm = rng.integers(0, P, (5, 142, 4), dtype=np.uint32)
    pr = rng.integers(0, P, (5, 26), dtype=np.uint32)
    pr[:, 0], pr[:, 1] = rng.integers(1, 24, 5), rng.integers(1, 24, 5)
    assert np.array_equal(rsv.oods_eval(sm, pr), ob.oods_eval(sm, pr))
    proof = read_proof("level13-1.bin")
    assert rsv.transcript(proof) == rsv._parse_transcript(ob.transcript_raw(proof))


# ---------------------------------------------------------------- witness: ws_witness, ws_inputs, the caller's scratch
_VARS = {}


def _oracle_variables(name):
    if name not in _VARS:
        from oracle import recursion_circuit as rc
        c, _, _ = rc.build_circuit(read_proof(name), ob, inputs_of(name))
        _VARS[name] = np.array(c.variables, dtype=np.uint32)
    return _VARS[name]


WITNESS_FORMS = ((None, 1, 0), (1, 0, 1), (1, 0, 2), (0, 0, 0))   # one launch; a launch per level with its strip; walking; the default rule


@pytest.mark.parametrize("layout", ["by_proof", "by_variable"])
@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_witness_of_three_with_the_middle_one_tampered(rsv, knobs, byte, layout):
    """The level2-1 template, 3 proofs with the middle one tampered, both layouts, in the one-launch, per-level and walking
    forms (forced as tests/test_witness_gpu.py forces them): the rows of the accepted proofs are the gadgets' vector."""
    import torch
    from tests.chain_harness import launch_form
    name = "level2-1.bin"
    want = _oracle_variables(name)
    proof = read_proof(name)
    batch, n = [proof, ob.tamper(proof, 5), proof], 3
    ctx = _context(rsv, knobs, byte)
    ctx.set_option("witness_layout", layout)
    wp = rsv.WitnessProgram.build(proof, fixture_cfg(name), inputs_of(name))
    d_blob, d_off = _to_dev(batch, rsv)
    for form in WITNESS_FORMS:
        d_vars = _filled(byte, (wp.n_vars, n, 4) if layout == "by_variable" else (n, wp.n_vars, 4))
        d_acc = _filled(byte, (n,), torch.uint8)
        with launch_form(ctx, form, n):
            ctx.witness(wp, d_blob, d_off, n, d_vars, d_acc, inputs=inputs_of(name))
            ctx.synchronize()
        got = u32(d_vars)
        got = got.transpose(1, 0, 2) if layout == "by_variable" else got
        assert d_acc.cpu().tolist() == [1, 0, 1], form
        assert np.array_equal(got[0], want) and np.array_equal(got[2], want), form
    ctx.close()
    wp.close()


_INNER = {}


def _inner_proofs(rsv, ctx):
    """Three genuine proofs of S1 under S1_CONFIG with the statements 11, 18 and 25, made by the chain once per session (on
    whatever context the first caller has; tests/test_verify_inputs_gpu.py asserts that these three verify), their
    statements, and the oracle's circuits that verify them."""
    if not _INNER:
        builts = _s1_witnesses()
        circ = _s1_circuit(rsv)
        ch, cfg, _ = _s1_chain(rsv, ctx, circ, *_s1_inputs())
        proofs = ch.proofs()
        circ.close()
        assert all(p is not None for p in proofs)
        inputs = [b.inputs for b in builts]
        assert _oracle_each(proofs, cfg, inputs) == ([1, 1, 1], [0, 0, 0])
        _INNER.update(proofs=proofs, inputs=inputs, cfg=cfg, own=np.stack([_records(i[3:]) for i in inputs]), rows={}, groups={})
    return _INNER


def _records(inputs):
    """[(idx, (v0, v1, v2, v3))] -> uint32[n, 5], the records Context.witness takes as d_inputs."""
    return np.array([[i, *v] for i, v in inputs], dtype=np.uint32).reshape(-1, 5)


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_witness_with_own_inputs_hashed_and_a_group_of_two(rsv, knobs, byte):
    """ws_inputs (the record array of the verifying pass, the shared records, the statements, the flags) and ws_witness under
    the programs that take every proof's own public input: the plain one and the hashed one on [proof 0, proof 1 tampered,
    proof 2], and the hashed program of two copies on the groups (0, 1) and (2, tampered 0).  The rows of the accepted
    proofs and of the accepted group are the oracle's circuits' variables, word for word."""
    import torch
    ctx = _context(rsv, knobs, byte)
    s = _inner_proofs(rsv, ctx)
    proofs, inputs, cfg = s["proofs"], s["inputs"], s["cfg"]
    fixed = inputs[0][:3]
    bad1, bad0 = ob.tamper(proofs[1], 7), ob.tamper(proofs[0], 7)
    assert _oracle_each([bad1, bad0], cfg, [inputs[1], inputs[0]])[0] == [0, 0]
    # rsv_verify_batch_inputs_dev (d_pi_sum): the three proofs under their own statements, the middle one tampered (rejected
    # behind the parser), then each proof under its neighbour's statement
    batch, d_rec = [proofs[0], bad1, proofs[2]], dev(np.stack([_records(i) for i in inputs]))
    assert _verify_ctx(rsv, ctx, batch, cfg, byte, d_inputs=d_rec, n_inputs=4) == _oracle_each(batch, cfg, inputs)
    rotated = inputs[1:] + inputs[:1]
    d_rot = dev(np.stack([_records(i) for i in rotated]))
    want = _oracle_each(proofs, cfg, rotated)
    assert want[0] == [0, 0, 0] and _verify_ctx(rsv, ctx, proofs, cfg, byte, d_inputs=d_rot, n_inputs=4) == want
    assert _verify_ctx(rsv, ctx, proofs, cfg, byte, d_inputs=d_rec, n_inputs=4) == ([1, 1, 1], [0, 0, 0])
    for hashed in (False, True):
        wp = rsv.WitnessProgram.build(proofs[0], cfg, inputs[0], n_fixed=3, hashed=hashed)
        F, S_ = wp.shape.flow_count, wp.stmt_flow
        d_blob, d_off = _to_dev([proofs[0], bad1, proofs[2]], rsv)
        d_own = dev(s["own"])
        d_vars, d_acc, d_reason = _filled(byte, (3, wp.n_vars, 4)), _filled(byte, (3,), torch.uint8), _filled(byte, (3,), torch.uint8)
        d_flow, d_swap = _filled(byte, (3 * (F + S_), 32)), _filled(byte, (3 * (F + S_),), torch.uint8)
        ctx.witness(wp, d_blob, d_off, 3, d_vars, d_acc, d_reason, inputs=fixed, d_flow=d_flow, d_flow_swap=d_swap, d_inputs=d_own)
        ctx.synchronize()
        got = u32(d_vars)
        assert d_acc.cpu().tolist() == [1, 0, 1] and d_reason.cpu().tolist()[0::2] == [0, 0], hashed
        for i in (0, 2):
            if (hashed, i) not in s["rows"]:
                c = ST.group_circuit([proofs[i]], [inputs[i]], 3) if hashed else WI.build_circuit(proofs[i], inputs[i], 3)[0]
                s["rows"][hashed, i] = np.array(c.variables, dtype=np.uint32)
            assert np.array_equal(got[i], s["rows"][hashed, i]), (hashed, i)
        if hashed:   # the statement hash's records behind the members'
            tail = u32(d_flow)[3 * F:].reshape(3, S_, 32)
            for i in (0, 2):
                assert np.array_equal(tail[i], ST.flow_records([int(s["own"][i, 0, 1])])), i
        wp.close()
    wp2 = rsv.WitnessProgram.build(proofs[0], cfg, inputs[0], copies=2, n_fixed=3, hashed=True)
    F, S_ = wp2.shape.flow_count, wp2.stmt_flow
    members = [proofs[0], proofs[1], proofs[2], bad0]
    d_blob, d_off = _to_dev(members, rsv)
    d_own = dev(s["own"][[0, 1, 2, 0]])
    total = 2 * (2 * F + S_)
    d_vars, d_acc = _filled(byte, (2, wp2.n_vars, 4)), _filled(byte, (2,), torch.uint8)
    d_macc, d_mreason = _filled(byte, (4,), torch.uint8), _filled(byte, (4,), torch.uint8)
    d_flow, d_swap = _filled(byte, (total, 32)), _filled(byte, (total,), torch.uint8)
    ctx.witness_groups(wp2, d_blob, d_off, 2, d_vars, d_acc, d_macc, d_mreason, inputs=fixed, d_flow=d_flow, d_flow_swap=d_swap, d_inputs=d_own)
    ctx.synchronize()
    assert d_acc.cpu().tolist() == [1, 0] and d_macc.cpu().tolist() == [1, 1, 1, 0]
    if "01" not in s["groups"]:
        s["groups"]["01"] = np.array(ST.group_circuit(proofs[:2], inputs[:2], 3).variables, dtype=np.uint32)
    assert np.array_equal(u32(d_vars)[0], s["groups"]["01"])
    wp2.close()
    ctx.close()


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_trace_and_interaction_outside_the_chain(rsv, knobs, byte):
    """The smallest fixture pair, three proofs with the middle one rejected, through the generic calls: Context.witness and
    Context.witness_trace give the 12 + 48 trace columns and the op column of the oracle's circuit (built on the CPU from the
    fixture alone), zeros for the rejected proof; Context.witness_interaction under the next fixture's (z, alpha) gives the
    restatement's 8 + 8 interaction columns and claimed sums from the oracle's columns, zeros and ok = 0 for the rejected one."""
    import torch
    from tests import interaction_ref as R
    from tests.chain_harness import lookup_of, oracle_columns
    pin = pin_of("small_proof.bin")
    src, dst = pin["src"], pin["dst"]
    ppre, plonk, qpre, poseidon, lp, lq, _ = oracle_columns(src)
    z, alpha = lookup_of(dst)
    if "interaction" not in _INNER_REF:
        _INNER_REF["interaction"] = R.interaction(ppre, plonk, qpre, poseidon, z, alpha, lp, lq)
    cp, cq, sums, ok = _INNER_REF["interaction"]
    assert ok
    proof, n = read_proof(src), 3
    ctx = _context(rsv, knobs, byte)
    wp = program_of(rsv, pin)
    _, wops = wp.gates()
    F = wp.shape.flow_count
    d_blob, d_off = _to_dev([proof, ob.tamper(proof, 5), proof], rsv)
    d_vars, d_acc = _filled(byte, (n, wp.n_vars, 4)), _filled(byte, (n,), torch.uint8)
    d_flow, d_swap = _filled(byte, (n, F, 32)), _filled(byte, (n, F), torch.uint8)
    ctx.witness(wp, d_blob, d_off, n, d_vars, d_acc, inputs=inputs_of(src), d_flow=d_flow, d_flow_swap=d_swap)
    d_plonk, d_poseidon, d_ops = _filled(byte, (n, 12, 1 << lp)), _filled(byte, (n, 48, 1 << lq)), _filled(byte, (n, max(len(wops), 1)))
    ctx.witness_trace(wp, d_vars, d_acc, n, d_plonk=d_plonk, d_poseidon=d_poseidon, d_ops=d_ops, d_flow=d_flow, d_flow_swap=d_swap)
    d_lookup = dev(np.tile(np.array(list(z) + list(alpha), np.uint32), (n, 1)))
    d_ip, d_iq, d_sums, d_ok = _filled(byte, (n, 8, 1 << lp)), _filled(byte, (n, 8, 1 << lq)), _filled(byte, (n, 2, 4)), _filled(byte, (n,), torch.uint8)
    ctx.witness_interaction(wp, d_plonk, d_poseidon, d_acc, d_lookup, n, d_ip, d_iq, d_sums, d_ok)
    ctx.synchronize()
    got = {k: u32(v) for k, v in (("plonk", d_plonk), ("poseidon", d_poseidon), ("ops", d_ops), ("ip", d_ip), ("iq", d_iq), ("sums", d_sums))}
    acc, okd = d_acc.cpu().tolist(), d_ok.cpu().tolist()
    ctx.close()
    wp.close()
    assert acc == [1, 0, 1] and okd == [1, 0, 1]
    for k in range(n):
        if k == 1:
            assert not any(got[key][k].any() for key in got)
            continue
        assert np.array_equal(got["plonk"][k], (plonk % P).astype(np.uint32)) and np.array_equal(got["poseidon"][k], (poseidon % P).astype(np.uint32)), k
        if len(wops):
            assert np.array_equal(got["ops"][k][:len(wops)], (ppre[3, wops[:, 0]] % P).astype(np.uint32)), k
        assert np.array_equal(got["ip"][k], cp.astype(np.uint32)) and np.array_equal(got["iq"][k], cq.astype(np.uint32)), k
        assert got["sums"][k].tolist() == [list(sums[0]), list(sums[1])], k


_INNER_REF = {}


def _run_quotients(ctx, groups, gpoints, b, n, points, samples, after, mask, shared, byte, source=0):
    gs = [{"log_size": log, "d_cols": dev(cols), "n_cols": cols.shape[-2], "proof_stride": 0 if i in shared else cols.shape[-2] << log}
          for i, (log, cols) in enumerate(groups)]
    d_quot = _filled(byte, (n, sum(4 << (log + b) for log in {log for log, _ in groups})))
    d_mask, d_points, d_samples, d_after = mask_dev(mask), dev(points), dev(samples), dev(after)
    ctx.fri_quotients(gs, gpoints, n, b, d_points, points.shape[1], d_samples, d_after, d_quot, d_mask=d_mask, source=source)
    ctx.synchronize()
    return u32(d_quot)


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_fri_quotients_smallest_cases(rsv, knobs, byte):
    """fri_ref.QCASES' masked case (three column sizes, three proofs, the middle one masked) and its shared group, from the
    evaluations and from the coefficients: every word of d_quot is the restatement's, a masked proof is zero."""
    ctx = _context(rsv, knobs, byte)
    for k, case in enumerate(("three_sizes_A_below_B", "shared_group")):
        b, n, mask, spec = F.QCASES[case]
        groups, gp, points, samples, after = F.qinputs(np.random.default_rng(4900 + k), spec, n)
        shared = {i for i, g in enumerate(spec) if g[2]}
        got = _run_quotients(ctx, groups, gp, b, n, points, samples, after, mask, shared, byte)
        coeffs = [(log, C.interpolate(cols, log)) for log, cols in groups]
        again = _run_quotients(ctx, coeffs, gp, b, n, points, samples, after, mask, shared, byte, source=rsv.SAMPLE_COEFFS)
        assert np.array_equal(got, again), case
        for p in range(n):
            if mask is not None and not mask[p]:
                assert not got[p].any(), (case, p)
                continue
            mine = [(log, cols[0 if i in shared else p]) for i, (log, cols) in enumerate(groups)]
            assert np.array_equal(got[p], F.ref_quotients(mine, gp, b, points[p], samples[p], after[p])), (case, p)
    ctx.close()


# ---------------------------------------------------------------- the chain of a fixture pair, every stage's workspace
@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_chain_of_the_smallest_pair_outputs_the_next_fixture(rsv, knobs, byte):
    """small_proof.bin -> recursive_proof_16_15.bin, three proofs with the middle one tampered (every stage masks it):
    Chain.proofs() and Chain.pack() are the next fixture byte for byte, None / empty for the rejected one."""
    pin = pin_of("small_proof.bin")
    src, dst = pin["src"], pin["dst"]
    cfg, want = fixture_cfg(dst), read_proof(dst)
    proof = read_proof(src)
    ctx = _context(rsv, knobs, byte)
    wp = program_of(rsv, pin)
    ch = chain(rsv, ctx, wp, [proof, ob.tamper(proof, 5), proof], inputs_of(src), cfg.log_blowup_factor, upto="fri", caps=True,
               log_last=cfg.log_last_layer_degree_bound)
    tail(ch, cfg)
    got = ch.proofs()
    blob, offsets = ch.pack(exact=True)
    blob, off = blob.cpu().numpy(), offsets.cpu().tolist()
    ctx.close()
    wp.close()
    assert got[1] is None and got[0] == want and got[2] == want
    assert off == [0, len(want), len(want), 2 * len(want)] and blob.tobytes() == want + want


# ---------------------------------------------------------------- chain stages through the generic calls
def _groups_dev(groups, shared=()):
    gs = []
    for i, (log, cols) in enumerate(groups):
        cols = np.ascontiguousarray(np.asarray(cols, dtype=np.int64) % P, dtype=np.uint32)
        gs.append({"log_size": log, "d_cols": dev(cols), "n_cols": cols.shape[1], "proof_stride": 0 if i in shared else cols.shape[1] << log})
    return gs


def _random_groups(spec, n, seed):
    rng = np.random.default_rng(seed)
    groups = [(log, rng.integers(0, P, (1 if sh else n, nc, 1 << log))) for log, nc, sh in spec]
    return groups, {i for i, (_, _, sh) in enumerate(spec) if sh}, rng


def _check_commit(ctx, spec, b, n, mask, seed, byte=0xFF):
    """Context.commit_tree on a random tree: roots, d_coeffs and d_lde are the restatement's, a masked proof gets zeros."""
    groups, shared, _ = _random_groups(spec, n, seed)
    gs = _groups_dev(groups, shared)
    for g in gs:
        g["d_coeffs"] = _filled(byte, (n, g["n_cols"], 1 << g["log_size"]))
        g["d_lde"] = _filled(byte, (n, g["n_cols"], 1 << (g["log_size"] + b)))
    d_roots, d_mask = _filled(byte, (n, 8)), mask_dev(mask)   # (held until the call is over: it is only enqueued)
    ctx.commit_tree(gs, n, b, d_roots, d_mask)
    ctx.synchronize()
    roots = u32(d_roots)
    for p in range(n):
        if mask is not None and not mask[p]:
            assert not roots[p].any() and all(not u32(g["d_coeffs"])[p].any() and not u32(g["d_lde"])[p].any() for g in gs), (spec, p)
            continue
        mine = [(log, cols[0 if i in shared else p]) for i, (log, cols) in enumerate(groups)]
        for (log, cols), g in zip(mine, gs):
            co = u32(g["d_coeffs"])[p]
            assert np.array_equal(co, C.interpolate(cols, log)), (spec, p)
            assert np.array_equal(u32(g["d_lde"])[p], C.evaluate(co, log, log + b)), (spec, p)
        assert roots[p].tolist() == C.commit(mine, b, ob).tolist(), (spec, p)


def _check_sample(ctx, spec, n, mask, seed, k, source=0, byte=0xFF, b=1):
    """Context.sample_tree on a random tree at k points per proof, from the columns (source 0) or from the coefficients a
    commit_tree of the same groups left (source 1): every value is the restatement's, a masked proof is zero."""
    groups, shared, rng = _random_groups(spec, n, seed)
    gs = _groups_dev(groups, shared)
    if source:
        with_cf = [dict(g, d_coeffs=_filled(byte, (n, g["n_cols"], 1 << g["log_size"]))) for g in gs]
        d_roots, d_mask = _filled(byte, (n, 8)), mask_dev(mask)   # (held until the call is over: it is only enqueued)
        ctx.commit_tree(with_cf, n, b, d_roots, d_mask)
        ctx.synchronize()
        gs = [{"log_size": g["log_size"], "d_cols": g["d_coeffs"], "n_cols": g["n_cols"]} for g in with_cf]
    pts = rng.integers(0, P, (n, k, 8)).astype(np.uint32)
    d_out, d_pts, d_mask = _filled(byte, (n, k, sum(g["n_cols"] for g in gs), 4)), dev(pts), mask_dev(mask)
    ctx.sample_tree(gs, n, d_pts, k, d_out, d_mask=d_mask, source=source)
    ctx.synchronize()
    got = u32(d_out)
    for p in range(n):
        if mask is not None and not mask[p]:
            assert not got[p].any(), (spec, p)
            continue
        mine = [(log, cols[0 if i in shared else p]) for i, (log, cols) in enumerate(groups)]
        want = S.sample_tree(mine, [(tuple(int(v) for v in pts[p, j, :4]), tuple(int(v) for v in pts[p, j, 4:])) for j in range(k)])
        assert np.array_equal(got[p], want), (spec, p)


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_commit_tree_cases(rsv, knobs, byte):
    """chain_harness.CASES (shared groups, masks, logs 0 .. 7) through one filled context."""
    ctx = _context(rsv, knobs, byte)
    for case, (spec, b, n, mask) in enumerate(CASES):
        _check_commit(ctx, spec, b, n, mask, 4100 + case, byte)
    ctx.close()


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_sample_tree_switches_and_the_budget_case(rsv, knobs, byte):
    """sample_ref.SWITCHES[1] and [3] (masks; [3] has more than one chunk per column, whose sums k_sp_finish adds and which
    k_sp_dot leaves unwritten for the masked proof), both sources; and 41 proofs with three masked under a 1 MB budget: the
    batch is cut into passes that carve the workspace again."""
    ctx = _context(rsv, knobs, byte)
    for case in (1, 3):
        spec, b, n, mask = S.SWITCHES[case]
        for source in (0, 1):
            _check_sample(ctx, spec, n, mask, 4200 + case, 4 if case == 1 else 2, source, byte, b)
    ctx.set_option("ws_budget_mb", 1)
    mask = [0 if p in (0, 20, 40) else 1 for p in range(41)]
    for source in (0, 1):
        _check_sample(ctx, [(9, 6, False), (8, 11, True)], 41, mask, 4290, 4, source, byte)
    ctx.close()


def _check_decommit(rsv, ctx, spec, b, n, mask, nq, seed, byte=0xFF):
    """Context.decommit_tree on a random tree at nq queries per proof with duplicates and a sibling pair, without a cap,
    writing one and reading it: values, witness nodes, their counts and the cap are the restatement's, zero past the counts
    and for a masked proof."""
    groups, shared, rng = _random_groups(spec, n, seed)
    gs = _groups_dev(groups, shared)
    q = rng.integers(0, 1 << 32, (n, nq)).astype(np.uint32)
    q[:, nq // 2:] = q[:, :nq - nq // 2]
    q[:, 1] = q[:, 0] ^ 1
    vcap, wcap = rsv.decommit_sizes(gs, b, nq)
    d_q, d_mask, d_cap = dev(q), mask_dev(mask), _filled(byte, (n, 2 << b, 8))
    runs = []
    for mode in (rsv.CAP_NONE, rsv.CAP_WRITE, rsv.CAP_READ):
        o = [_filled(byte, (n, vcap)), _filled(byte, (n,)), _filled(byte, (n, wcap, 8)), _filled(byte, (n,))]
        ctx.decommit_tree(gs, n, b, d_q, nq, *o, d_mask=d_mask, cap_mode=mode, d_cap=None if mode == rsv.CAP_NONE else d_cap)
        ctx.synchronize()
        runs.append([u32(t) for t in o])
    cap = u32(d_cap)
    for values, nv, wit, nw in runs:
        for p in range(n):
            if mask is not None and not mask[p]:
                assert nv[p] == 0 and nw[p] == 0 and not values[p].any() and not wit[p].any() and not cap[p].any(), (spec, p)
                continue
            mine = [(log, cols[0 if i in shared else p]) for i, (log, cols) in enumerate(groups)]
            rv, rw, rcap = D.decommit(C.tree_layers(mine, b), q[p], ob, b)
            assert nv[p] == len(rv) and nw[p] == len(rw), (spec, p)
            assert np.array_equal(values[p, :nv[p]], rv) and not values[p, nv[p]:].any(), (spec, p)
            assert np.array_equal(wit[p, :nw[p]], rw) and not wit[p, nw[p]:].any(), (spec, p)
            assert np.array_equal(cap[p], rcap), (spec, p)


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_decommit_tree_cases(rsv, knobs, byte):
    """The second of chain_harness.CASES and its two masked ones (a shared group each), 7 queries."""
    ctx = _context(rsv, knobs, byte)
    for case in (1, 6, 7):
        spec, b, n, mask = CASES[case]
        _check_decommit(rsv, ctx, spec, b, n, mask, 7, 4600 + case, byte)
    ctx.close()


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_composition_smallest_shape_with_a_masked_proof(rsv, knobs, byte):
    """composition_ref.SHAPES[1], (lp, lq) = (3, 5), three proofs with the middle one masked: d_comp and d_comp_coeffs are the
    restatement's, zero for the masked proof."""
    lp, lq, n, mask, _ = K.SHAPES[1]
    rng = np.random.default_rng(4700)
    plonk = [rng.integers(0, P, (n, c, 1 << lp)) for c in (10, 12, 8)]
    poseidon = [rng.integers(0, P, (n, c, 1 << lq)) for c in (40, 48, 8)]
    sums, draws = rng.integers(0, P, (n, 2, 4)), rng.integers(0, P, (n, 12))
    L3 = rsv.composition_log_size(lp, lq)
    ctx = _context(rsv, knobs, byte)
    d_comp, d_co, d_mask = _filled(byte, (n, 8, 1 << L3)), _filled(byte, (n, 8, 1 << L3)), mask_dev(mask)
    dp, dq, d_sums, d_draws = [dev(c) for c in plonk], [dev(c) for c in poseidon], dev(sums), dev(draws)
    ctx.composition(lp, lq, dp, dq, d_sums, d_draws, n, d_comp, d_co, d_mask=d_mask)
    ctx.synchronize()
    comp, co = u32(d_comp), u32(d_co)
    ctx.close()
    for p in range(n):
        if not mask[p]:
            assert not comp[p].any() and not co[p].any()
            continue
        want, want_co = K.composition([c[p] for c in plonk], [c[p] for c in poseidon], lp, lq, sums[p], draws[p])
        assert np.array_equal(comp[p], want) and np.array_equal(co[p], want_co), p


def _check_fri(rsv, ctx, sizes, log_last, b, n, mask, seed, byte=0xFF, tail_log=0, sub_log=0):
    """Context.fri_commit (per layer; the tail form with tail_log; leaving the caps with sub_log) and Context.fri_open (from
    those caps with sub_log) on random quotient columns at one query per proof: roots, alphas, layers, last polynomial, flag,
    channel and both opening lists are the restatement's; a masked proof gets zeros."""
    import torch
    rng = np.random.default_rng(seed)
    cols = [{s: rng.integers(0, P, (4, 1 << s)) for s in sizes} for _ in range(n)]
    chan0 = np.zeros((n, 16), np.uint32)
    chan0[:, :9] = rng.integers(0, P, (n, 9))
    chan0[:, 8] %= 5
    queries = rng.integers(0, 1 << 32, (n, 1)).astype(np.uint32)   # bits above sizes[0] are ignored
    M, ni = sizes[0], F.n_inner_of(sizes[0], log_last, b)
    T, lw = 1 + ni, sum(4 << (sizes[0] - 1 - i) for i in range(ni))
    d_quot, chan = dev(np.stack([np.concatenate([c[s].reshape(-1) for s in sizes]) for c in cols])), dev(chan0)
    o = {"roots": _filled(byte, (n, T, 8)), "alphas": _filled(byte, (n, T, 4)), "layers": _filled(byte, (n, max(lw, 1))),
         "last": _filled(byte, (n, 1 << log_last, 4)), "low": _filled(byte, (n,), torch.uint8)}
    caps = _filled(byte, (max(rsv.fri_cap_sizes(sizes, b, log_last, sub_log, n)[0], 1),)) if sub_log else None
    d_mask, d_queries = mask_dev(mask), dev(queries)
    ctx.fri_commit(d_quot, sizes, b, log_last, n, chan, o["roots"], o["alphas"], o["layers"] if ni else None, o["last"], o["low"], d_mask=d_mask,
                   sub_log=sub_log, d_caps=caps, tail_log=tail_log)
    vcap, wcap = rsv.fri_open_sizes(sizes, b, log_last, 1)
    w = {"fw": _filled(byte, (n, T, vcap, 4)), "nf": _filled(byte, (n, T)), "hw": _filled(byte, (n, T, wcap, 8)), "nh": _filled(byte, (n, T))}
    ctx.fri_open(d_quot, o["layers"] if ni else None, sizes, b, log_last, n, d_queries, 1, w["fw"], w["nf"], w["hw"], w["nh"], d_mask=d_mask,
                 sub_log=sub_log, d_caps=caps)
    ctx.synchronize()
    got = {k: (v.cpu().numpy() if k == "low" else u32(v)) for k, v in {**o, **w}.items()}
    got["chan"] = u32(chan)
    for p in range(n):
        if mask is not None and not mask[p]:
            for k in ("roots", "alphas", "last", "chan", "fw", "nf", "hw", "nh") + (("layers",) if ni else ()):
                assert not got[k][p].any(), (k, p)
            assert got["low"][p] == 0
            continue
        ch = C.Channel(ob, chan0[p, :8], int(chan0[p, 8]))
        want = F.commit(cols[p], log_last, b, ch, ob)
        assert np.array_equal(got["roots"][p], want["roots"]) and np.array_equal(got["alphas"][p], want["alphas"]), p
        if ni:
            assert np.array_equal(got["layers"][p], np.concatenate([l.reshape(-1) for l in want["layers"]]).astype(np.uint32)), p
        assert np.array_equal(got["last"][p], want["last_poly"]) and got["low"][p] == want["low_degree"] == 0, p
        assert np.array_equal(got["chan"][p, :8], ch.digest) and got["chan"][p, 8] == ch.n_sent and not got["chan"][p, 9:].any()
        qs = [int(queries[p, 0]) & ((1 << M) - 1)]
        for t, (fw, hw, root) in enumerate(FO.open_all(cols[p], want["layers"], qs, ob)):
            nf, nh = int(got["nf"][p, t]), int(got["nh"][p, t])
            assert (nf, nh) == (len(fw), len(hw)), (p, t)
            assert np.array_equal(got["fw"][p, t, :nf], fw) and np.array_equal(got["hw"][p, t, :nh], hw), (p, t)
            assert not got["fw"][p, t, nf:].any() and not got["hw"][p, t, nh:].any(), (p, t)
            assert np.array_equal(got["roots"][p, t], root), (p, t)


@pytest.mark.parametrize("form", ["per_layer", "tail_2", "cap_1"])
@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_fri_commit_and_open(rsv, knobs, byte, form):
    """fri_ref.CCASES' masked case (columns of 2^6 and 2^4, three proofs, the middle one masked) and its first (three
    columns), per layer, in the tail form (t = 2) and leaving and reading the caps (h = 1), opened at one query."""
    kw = {"per_layer": {}, "tail_2": {"tail_log": 2}, "cap_1": {"sub_log": 1}}[form]
    ctx = _context(rsv, knobs, byte)
    for k, case in enumerate(("joins_at_the_last_fold", "three_columns")):
        sizes, log_last, b, n, mask, _ = F.CCASES[case]
        _check_fri(rsv, ctx, sizes, log_last, b, n, mask, 4800 + k, byte, **kw)
    ctx.close()


def _channels(seeds):
    out = np.zeros((len(seeds), 16), np.uint32)
    for k, s in enumerate(seeds):
        rng = np.random.default_rng(s)
        out[k, :8] = rng.integers(0, P, 8)
        out[k, 8] = rng.integers(1, 5)
    return out


def _check_grind(ctx, chans, pow_bits, mask, byte=0xFF):
    """Context.pow_grind against the restatement, proof by proof; a masked proof's nonce and channel are zero."""
    n = len(chans)
    d_chan, d_nonce, d_ok = dev(chans), _filled(byte, (n, 2)), mask_dev(mask)
    ctx.pow_grind(pow_bits, n, d_ok, d_chan, d_nonce)
    ctx.synchronize()
    nonce, after, ok = u32(d_nonce).astype(np.uint64), u32(d_chan), d_ok.cpu().numpy()
    for p, c in enumerate(chans):
        got = int(nonce[p, 0]) | int(nonce[p, 1]) << 32
        if not mask[p]:
            assert got == 0 and not after[p].any() and ok[p] == 0, p
            continue
        want = W.grind(c, pow_bits, 0, 1 << (pow_bits + 6), ob)
        assert want is not None and got == want, (p, got, want)
        assert np.array_equal(after[p], W.mix_nonce(c, want, ob)) and ok[p] == 1, p


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_pow_grind_and_draw_queries(rsv, knobs, byte):
    """8 bits, five proofs, one masked: the smallest nonce from 0 and the channel behind its mix.  `best` lives in ws_pow and
    is preset to all ones by the call; under fill 0x00 a missing preset leaves every nonce 0.  Then the queries drawn from
    those channels."""
    ctx = _context(rsv, knobs, byte)
    chans, mask = _channels((11, 12, 13, 14, 15)), [1, 1, 0, 1, 1]
    _check_grind(ctx, chans, 8, mask, byte)
    n, nq = len(chans), 9
    d_chan, d_q, d_low = dev(chans), _filled(byte, (n, nq)), _filled(byte, (n, nq))
    d_mask = mask_dev(mask)
    ctx.draw_queries(n, nq, 20, 13, d_chan, d_q, d_low, d_mask=d_mask)
    ctx.synchronize()
    after, q, low = u32(d_chan), u32(d_q), u32(d_low)
    ctx.close()
    for p in range(n):
        if not mask[p]:
            assert not after[p].any() and not q[p].any() and not low[p].any()
            continue
        wq, wlow, wafter = W.draw_queries(chans[p], nq, 20, 13, ob)
        assert np.array_equal(q[p], wq) and np.array_equal(low[p], wlow) and np.array_equal(after[p], wafter), p


def _pack(rsv, ctx, hdr, plist, mask=None, override=None, byte=0xFF):
    import torch
    n = len(plist)
    parts, keep = PR.lay(rsv, hdr, plist, PR.CAPS, override)
    d_blob = torch.full((n * rsv.proof_bytes_bound(hdr[4], hdr[6], PR.caps_list(PR.CAPS, hdr[6])),), byte, dtype=torch.uint8, device=DEV)
    d_offsets = _filled(byte, (n + 1,), torch.int64)
    d_mask = mask_dev(mask)
    ctx.proof_pack(parts, n, d_blob, d_offsets, d_mask=d_mask)
    ctx.synchronize()
    del keep
    return d_blob.cpu().numpy(), d_offsets.cpu().numpy().tolist()


def _check_pack(rsv, ctx, hdr, n, mask, over_slot, seed, byte=0xFF):
    """Random parts: per slot chain.proof_bytes' bytes, an empty slot for a masked proof and for one over capacity, the
    prefill behind."""
    rng = np.random.default_rng(seed)
    T, caps = hdr[6], PR.caps_list(PR.CAPS, hdr[6])
    plist = [PR.random_parts(rng, T, hdr[4], [int(rng.choice([0, 1, cap - 1, cap])) for cap in caps]) for _ in range(n)]
    over = {} if over_slot is None else {(over_slot, 9): caps[9] + 1}
    want = [b"" if (mask and not mask[k]) or k == over_slot else PR.expected(rsv, hdr, p) for k, p in enumerate(plist)]
    blob, offsets = _pack(rsv, ctx, hdr, plist, mask, over, byte)
    assert offsets == np.cumsum([0] + [len(w) for w in want]).tolist()
    for k, w in enumerate(want):
        assert blob[offsets[k]:offsets[k + 1]].tobytes() == w, k
    assert (blob[offsets[-1]:] == byte).all()


@pytest.mark.parametrize("byte", BYTES, ids=byte_id)
def test_proof_pack_random_parts(rsv, knobs, byte):
    """T = 2, n = 3, proof 0 masked and proof 1 over capacity."""
    ctx = _context(rsv, knobs, byte)
    _check_pack(rsv, ctx, (7, 6, 3, 1, 2, 2, 2), 3, [0, 1, 1], 1, 4400, byte)
    ctx.close()


# ---------------------------------------------------------------- the knob off: a different call in between
def test_verify_batch_with_another_configuration_in_between(rsv, knobs):
    """One context.  First small_proof.bin's configuration and recursive_proof_16_15.bin's (the same n_queries, log_last 2
    and 8), then two S1 configurations that differ in n_queries only (15 and 17): A with proofs 1 and 3 tampered, B larger
    with every proof accepted and another n, A' with fewer proofs and proof 0 tampered.  Every verdict is the oracle's."""
    from tests import verify_grid as G
    ctx = _context(rsv, knobs, None)
    programs = G.Programs(rsv)
    made = {nq: G.generate(rsv, ctx, ("S1", 2, 1, 0, nq), programs) for nq in (15, 17)}
    programs.close()
    small, rec = read_proof("small_proof.bin"), read_proof("recursive_proof_16_15.bin")
    pairs = [((small, fixture_cfg("small_proof.bin"), inputs_of("small_proof.bin")), (rec, fixture_cfg("recursive_proof_16_15.bin"), rsv.STANDARD_INPUTS)),
             (made[15], made[17])]
    for (pa, ca, ia), (pb, cb, ib) in pairs:
        for batch, cfg, inputs in (([pa, ob.tamper(pa, 1), pa, ob.tamper(pa, 2), pa], ca, ia), ([pb] * 7, cb, ib), ([ob.tamper(pa, 3), pa, pa], ca, ia)):
            oacc, oreason = ob.verify_batch(batch, cfg, inputs)
            assert _verify_ctx(rsv, ctx, batch, cfg, inputs=inputs) == (oacc.tolist(), oreason.tolist())
        assert oacc.tolist() == [0, 1, 1]
    ctx.close()


def test_sample_commit_pow_and_pack_with_another_call_in_between(rsv, knobs):
    """One context, the knob off.  sample_tree: a masked batch with several chunks per column, a larger unmasked one, the
    first shape again with fewer proofs and another mask.  commit_tree: the same log_size under another blow-up and back
    (the twiddle tables are cached by log size).  pow_grind: five proofs, seven, three with another mask.  proof_pack: two
    7-word keys alternating (the map is cached by the key)."""
    ctx = _context(rsv, knobs, None)
    _check_sample(ctx, [(14, 2, True), (13, 1, False)], 3, [1, 1, 0], 4500, 2)
    _check_sample(ctx, [(14, 3, False), (13, 2, False)], 4, None, 4501, 4)
    _check_sample(ctx, [(14, 2, True), (13, 1, False)], 2, [0, 1], 4502, 2)
    _check_commit(ctx, [(6, 5, True), (5, 7, False)], 2, 4, [1, 0, 1, 1], 4510)
    _check_commit(ctx, [(6, 5, False), (5, 7, False)], 4, 5, None, 4511)
    _check_commit(ctx, [(6, 5, True), (5, 7, False)], 2, 3, [1, 1, 0], 4512)
    _check_grind(ctx, _channels((21, 22, 23, 24, 25)), 8, [1, 0, 1, 1, 1])
    _check_grind(ctx, _channels(range(30, 37)), 9, [1] * 7)
    _check_grind(ctx, _channels((21, 22, 23)), 8, [0, 1, 1])
    key_a, key_b = (7, 6, 3, 1, 2, 2, 2), (7, 6, 3, 1, 0, 2, 5)
    _check_pack(rsv, ctx, key_a, 3, [0, 1, 1], 1, 4520)
    _check_pack(rsv, ctx, key_b, 6, None, None, 4521)
    _check_pack(rsv, ctx, key_a, 2, [1, 0], None, 4522)
    _check_pack(rsv, ctx, key_b, 2, [0, 1], None, 4523)
    ctx.close()


def test_witness_and_interaction_with_another_batch_in_between(rsv, knobs):
    """One context through the chain's commit stage (witness, trace, interaction, trees 0-2) of the smallest pair: three
    proofs with the middle one tampered, five accepted, two with the first tampered.  The roots of the accepted proofs are
    the next fixture's commitments and the sums its claimed sums; the rejected proofs' are flagged."""
    from oracle import recursion_circuit as rc
    pin = pin_of("small_proof.bin")
    src, dst = pin["src"], pin["dst"]
    d = rc.parse_proof(read_proof(dst))
    b = fixture_cfg(dst).log_blowup_factor
    proof = read_proof(src)
    ctx = _context(rsv, knobs, None)
    wp = program_of(rsv, pin)
    for batch in ([proof, ob.tamper(proof, 5), proof], [proof] * 5, [ob.tamper(proof, 9), proof]):
        good = [p == proof for p in batch]
        r = chain(rsv, ctx, wp, batch, inputs_of(src), b).numpy()
        assert r["acc"].tolist() == [int(g) for g in good] and r["ok"].tolist() == [int(g) for g in good]
        for k, g in enumerate(good):
            if g:
                assert r["roots"][k].tolist() == [[int(x) for x in d.commitments[t]] for t in range(3)], k
                assert tuple(r["sums"][k, 0].tolist()) == tuple(d.plonk_total_sum) and tuple(r["sums"][k, 1].tolist()) == tuple(d.poseidon_total_sum)
    ctx.close()
    wp.close()
