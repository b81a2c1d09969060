"""The host-pointer entry points on the device, through the one staging path they share (csrc/host_stage.inc): what that path
computes and no other test reached — a batch whose first proof does not start at byte 0, a host cfg_of, the refusals that
sit behind the device selection, every probe at one element and at one past a workgroup, its bad flag, and a correct call
after a refused one.  The status codes of the refusals were recorded from a build of commit b9e5200 (the parent of the
change that introduced the shared path), on which this whole file passes as well."""
import ctypes

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests.conftest import fixture_cfg, load_manifest, read_proof
from tests.test_gpu_parity import _row_from_raw, entry_inputs

pytestmark = pytest.mark.gpu

P = 0x7FFFFFFF
OK, NULL, SIZE, RANGE = 0, -1, -2, -5
SMALL = "small_proof.bin"
SMALL_INPUTS = [(1, (1, 0, 0, 0))]
JUNK = 7  # bytes in front of the first proof


def _shifted_pack(rsv):
    """rsv.pack with JUNK bytes in front of the blob and offsets[0] = JUNK: every binding function stages such a batch."""
    plain = rsv.pack

    def pack(proofs):
        blob, offsets = plain(proofs)
        return np.concatenate([np.full(JUNK, 0xA5, np.uint8), blob]), offsets + np.uint64(JUNK)
    return pack


def _small_shape():
    e = next(e for e in load_manifest() if e["file"] == SMALL)
    M = max(e["log_size_plonk"] + 1, e["log_size_poseidon"] + 2) + e["log_blowup_factor"]
    return e["n_queries"], M


def _hints(rsv, proofs, cfg, inputs):
    """rsv_verify_hints with a transcript and the trace paths asked for -> (status, transcript, sib, pos, accept, reason)."""
    nq, M = _small_shape()
    n = len(proofs)
    blob, offsets = rsv.pack(proofs)
    tr = np.zeros((n, rsv.TRANSCRIPT_WORDS), np.uint32)
    sib, pos = np.zeros((n, 4, nq, M, 8), np.uint32), np.zeros((n, 4, nq), np.uint32)
    acc, reason = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ho = rsv.HintsOut(n_queries=nq, max_log=M, d_transcript=tr.ctypes.data, d_trace_sib=sib.ctypes.data, d_trace_pos=pos.ctypes.data)
    items = list(inputs)
    rc = rsv.lib.rsv_verify_hints(blob.ctypes.data_as(rsv._u8p), offsets.ctypes.data_as(rsv._u64p), n, rsv.prepare_cfg(cfg, n).ref(),
                                  rsv.make_inputs(items), len(items), ctypes.byref(ho), acc.ctypes.data_as(rsv._u8p), reason.ctypes.data_as(rsv._u8p), 0)
    return rc, tr, sib, pos, acc, reason


@pytest.fixture(scope="module")
def small_program(rsv):
    wp = rsv.WitnessProgram.build(read_proof(SMALL), fixture_cfg(SMALL), SMALL_INPUTS)
    yield wp
    wp.close()


@pytest.fixture(scope="module")
def base0(rsv, small_program):
    """Every form on three proofs (genuine, tampered, genuine) that start at byte 0, each checked against the oracle as the
    existing parity tests state it; the non-zero-base calls are compared with these."""
    from oracle import recursion_circuit as rc
    small, cfg = read_proof(SMALL), fixture_cfg(SMALL)
    batch = [small, ob.tamper(small, 3), small]
    oacc, oreason = ob.verify_batch(batch, cfg, SMALL_INPUTS)
    out = {"batch": batch}
    out["verify"] = rsv.verify_batch(batch, cfg, SMALL_INPUTS)
    out["inputs"] = rsv.verify_batch(batch, cfg, inputs_per_proof=[SMALL_INPUTS] * 3)
    out["hints"] = _hints(rsv, batch, cfg, SMALL_INPUTS)
    out["witness"] = rsv.witness(batch, small_program, SMALL_INPUTS, with_flow=True)
    for acc, reason in (out["verify"], out["inputs"], out["hints"][4:], out["witness"][1:3]):
        assert acc.tolist() == oacc.tolist() == [1, 0, 1] and reason.tolist() == oreason.tolist()
    rc_h, tr, sib, pos, _, _ = out["hints"]
    assert rc_h == OK
    nq, M = _small_shape()
    for i, pr in enumerate(batch):
        assert np.array_equal(tr[i], _row_from_raw(ob.transcript_raw(pr))), i
    osib, opos, depth = ob.trace_paths(small, nq, M, SMALL_INPUTS)
    for k in (0, 2):
        assert np.array_equal(pos[k], opos)
        for t in range(4):
            d = int(depth[t])
            assert np.array_equal(sib[k, t, :, :d, :], osib[t, :, :d, :]), (k, t)
    c, _, _ = rc.build_circuit(small, ob, SMALL_INPUTS)
    assert np.array_equal(out["witness"][0][0], np.array(c.variables, dtype=np.uint32))
    return out


def _same(a, b):
    return all((x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [1, 3])
def test_a_batch_that_does_not_start_at_byte_0(rsv, monkeypatch, small_program, base0, n):
    """JUNK bytes in front of the blob, offsets[0] = JUNK: accept, reason and every output of the four batch forms are
    byte-equal to the same call with base 0 (which equals the oracle: base0)."""
    cfg, batch = fixture_cfg(SMALL), base0["batch"][:n]
    first = {"verify": rsv.verify_batch(batch, cfg, SMALL_INPUTS), "inputs": rsv.verify_batch(batch, cfg, inputs_per_proof=[SMALL_INPUTS] * n),
             "hints": _hints(rsv, batch, cfg, SMALL_INPUTS), "witness": rsv.witness(batch, small_program, SMALL_INPUTS, with_flow=True)}
    for k, v in first.items():  # (the first n proofs of base0's batch: the same rows)
        assert _same([x[:n] for x in v if isinstance(x, np.ndarray)], [x[:n] for x in base0[k] if isinstance(x, np.ndarray)]), k
    monkeypatch.setattr(rsv, "pack", _shifted_pack(rsv))
    blob, offsets = rsv.pack(batch)
    assert int(offsets[0]) == JUNK and len(blob) == JUNK + sum(len(p) for p in batch)
    assert _same(rsv.verify_batch(batch, cfg, SMALL_INPUTS), first["verify"])
    assert _same(rsv.verify_batch(batch, cfg, inputs_per_proof=[SMALL_INPUTS] * n), first["inputs"])
    shifted = _hints(rsv, batch, cfg, SMALL_INPUTS)
    assert shifted[0] == OK and _same(shifted[1:], first["hints"][1:])
    assert _same(rsv.witness(batch, small_program, SMALL_INPUTS, with_flow=True), first["witness"])


def test_two_proofs_under_two_configurations(rsv):
    """A host cfg_of through rsv_verify_batch and rsv_verify_hints: the two smallest fixtures whose configurations differ,
    in both orders and each under the other's configuration; the verdicts are the _dev path's."""
    import torch
    by_size = sorted((e for e in load_manifest() if e["expect"] == "ok"), key=lambda e: len(read_proof(e["file"])))
    a = by_size[0]
    b = next(e for e in by_size[1:] if rsv._cfg_key(fixture_cfg(e["file"])) != rsv._cfg_key(fixture_cfg(a["file"])))
    assert (a["file"], b["file"]) == (SMALL, "level12-1.bin")
    pa, pb, ca, cb = read_proof(a["file"]), read_proof(b["file"]), fixture_cfg(a["file"]), fixture_cfg(b["file"])
    ia, ib = entry_inputs(a), entry_inputs(b)
    ctx = rsv.Context(0)
    for proofs, cfgs, inputs in (([pa, pb], [ca, cb], ia), ([pb, pa], [cb, ca], ib), ([pa, pb], [cb, ca], ia)):
        pc = rsv.prepare_cfg(cfgs, 2)
        assert pc.struct.n_cfgs == 2 and pc.struct.cfg_of
        acc, reason = rsv.verify_batch(proofs, cfgs, inputs)
        blob, offsets = rsv.pack(proofs)
        tr, hacc, hreason = np.zeros((2, rsv.TRANSCRIPT_WORDS), np.uint32), np.zeros(2, np.uint8), np.zeros(2, np.uint8)
        ho = rsv.HintsOut(d_transcript=tr.ctypes.data)
        assert rsv.lib.rsv_verify_hints(blob.ctypes.data_as(rsv._u8p), offsets.ctypes.data_as(rsv._u64p), 2, pc.ref(), rsv.make_inputs(inputs), len(inputs),
                                        ctypes.byref(ho), hacc.ctypes.data_as(rsv._u8p), hreason.ctypes.data_as(rsv._u8p), 0) == OK
        dev = torch.device("cuda:0")
        d_blob, d_off = torch.from_numpy(blob.copy()).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)
        d_acc, d_reason = torch.zeros(2, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.uint8, device=dev)
        ctx.verify_batch(d_blob, d_off, 2, d_acc, d_reason, cfg=cfgs, inputs=inputs)
        ctx.synchronize()
        want = (d_acc.cpu().numpy().tolist(), d_reason.cpu().numpy().tolist())
        assert (acc.tolist(), reason.tolist()) == want and (hacc.tolist(), hreason.tolist()) == want
        oacc, oreason = ob.verify_batch(proofs, cfgs, inputs)
        assert want == (oacc.tolist(), oreason.tolist())
        assert np.array_equal(tr, rsv.transcript_batch(proofs, cfgs))
    ctx.close()


SENTINEL = 0xC3


def _batch_calls(rsv, program, proofs, offsets=None, n=None, hints=None):
    """The four batch forms over `proofs` with the offsets (and n) given instead of the packed ones -> {form: (status, outputs)};
    every output array starts as SENTINEL bytes."""
    blob, packed = rsv.pack(proofs)
    offsets = packed if offsets is None else np.asarray(offsets, np.uint64)
    n = len(proofs) if n is None else n
    cfg, nq_M = rsv.prepare_cfg(fixture_cfg(SMALL), max(n, 1)), _small_shape()
    m = max(len(proofs), 1)
    u8, u32 = (lambda *s: np.full(s, SENTINEL, np.uint8)), (lambda *s: np.full(s, SENTINEL * 0x01010101, np.uint32))
    pi = rsv.make_inputs(SMALL_INPUTS)
    lead = (blob.ctypes.data_as(rsv._u8p), offsets.ctypes.data_as(rsv._u64p), n, cfg.ref(), pi, 1)
    res = {}
    out = [u8(m), u8(m)]
    res["rsv_verify_batch"] = (rsv.lib.rsv_verify_batch(*lead, out[0].ctypes.data_as(rsv._u8p), out[1].ctypes.data_as(rsv._u8p), 0), out)
    out = [u8(m), u8(m)]
    own = rsv.make_inputs(SMALL_INPUTS * m)
    res["rsv_verify_batch_inputs"] = (rsv.lib.rsv_verify_batch_inputs(*lead[:4], own, 1, out[0].ctypes.data_as(rsv._u8p), out[1].ctypes.data_as(rsv._u8p), 0), out)
    out = [u8(m), u8(m), u32(m, rsv.TRANSCRIPT_WORDS), u32(m, 4, nq_M[0], nq_M[1], 8), u32(m, 4, nq_M[0]), u32(m, 64, 32), u8(m, 64)]
    ho = rsv.HintsOut(**(hints(out) if hints else dict(n_queries=nq_M[0], max_log=nq_M[1], d_transcript=out[2].ctypes.data,
                                                      d_trace_sib=out[3].ctypes.data, d_trace_pos=out[4].ctypes.data)))
    res["rsv_verify_hints"] = (rsv.lib.rsv_verify_hints(*lead, ctypes.byref(ho), out[0].ctypes.data_as(rsv._u8p), out[1].ctypes.data_as(rsv._u8p), 0), out)
    out = [u8(m), u8(m), u32(m, program.n_vars, 4)]
    res["rsv_witness_eval"] = (rsv.lib.rsv_witness_eval(program._h, *lead, out[2].ctypes.data_as(rsv._u32p), None, None, out[0].ctypes.data_as(rsv._u8p),
                                                        out[1].ctypes.data_as(rsv._u8p), 0), out)
    return res


def _untouched(outs):
    return all((o.view(np.uint8) == SENTINEL).all() for o in outs)


def test_refusals_behind_the_device_and_a_correct_call_after_each(rsv, small_program, base0):
    """A decreasing offset pair in each of the four batch forms, a hints output with no declared shape, d_flow_swap with
    flow_stride 0: RSV_E_SIZE, no output written; an empty batch: RSV_OK, no output written.  After every refused call the
    same process makes a correct one: the refused call's context and buffers were torn down cleanly."""
    small = read_proof(SMALL)
    batch, L = base0["batch"], len(small)

    def correct_call_follows():
        acc, reason = rsv.verify_batch(batch, fixture_cfg(SMALL), SMALL_INPUTS)
        assert _same((acc, reason), base0["verify"])
        assert _same(rsv.witness(batch[:1], small_program, SMALL_INPUTS), [x[:1] for x in base0["witness"][:3]])

    for offsets in ([0, L, L - 4, 3 * L], [4, 0, L, 2 * L], [0, L, 2 * L, 2 * L - 4]):  # a pair in the middle, the first, the last
        for form, (rc, outs) in _batch_calls(rsv, small_program, batch, offsets=offsets).items():
            assert rc == SIZE and _untouched(outs), (form, offsets)
        correct_call_follows()
    # a hints output without a declared shape (trace_sib with n_queries = max_log = 0), and d_flow_swap with flow_stride 0
    for hints in (lambda o: dict(d_trace_sib=o[3].ctypes.data, d_trace_pos=o[4].ctypes.data),
                  lambda o: dict(d_flow=o[5].ctypes.data, d_flow_swap=o[6].ctypes.data, flow_stride=0),
                  lambda o: dict(d_transcript=o[2].ctypes.data, d_flow=o[5].ctypes.data, d_flow_swap=o[6].ctypes.data, flow_stride=0)):
        rc, outs = _batch_calls(rsv, small_program, batch, hints=hints)["rsv_verify_hints"]
        assert rc == SIZE and _untouched(outs)
        correct_call_follows()
    # the empty batch (for the witness form ahead of the device, for the verify forms behind it)
    for form, (rc, outs) in _batch_calls(rsv, small_program, [], offsets=[0], n=0).items():
        assert rc == OK and _untouched(outs), form
    correct_call_follows()


def _probe_cases(rsv, n, seed):
    """name -> (call returning the output, the oracle's output) for the ten array probes at n elements."""
    rng = np.random.default_rng(seed)
    r = lambda *shape: rng.integers(0, P, shape, dtype=np.uint32)
    st, l8, r8, sw, sw3 = r(n, 16), r(n, 8), r(n, 8), rng.integers(0, 2, n, dtype=np.uint8), rng.integers(0, 3, n).astype(np.uint8)
    cols = r(n, 13)
    depth, n_cols_at = 5, [0, 3, 0, 0, 0, 9]
    q, sib, pcols = rng.integers(0, 1 << depth, n, dtype=np.uint32), r(n, depth, 8), r(n, 12)
    a4, b4, dq = r(n, 4), r(n, 4), rng.integers(0, 1 << 13, n, dtype=np.uint32)
    coeffs, xs = r(8, 4), r(n)
    good = ob.line_eval(coeffs, xs)
    folded = good.copy()
    folded[::2, 1] = (folded[::2, 1] + 1) % P
    sm, pr = r(n, 142, 4), r(n, 26)
    pr[:, 0], pr[:, 1] = rng.integers(1, 27, n), rng.integers(1, 27, n)
    return {
        "rsv_poseidon2_permute": (lambda: rsv.poseidon2_permute(st), ob.poseidon2_permute(st)),
        "rsv_poseidon2_half_permute": (lambda: np.stack(rsv.half_permute(l8, r8, sw)), np.stack(ob.half_permute(l8, r8, sw))),
        "rsv_poseidon2_emulated": (lambda: rsv.poseidon2_emulated(l8, r8, sw3), ob.emulated_rows(l8, r8, sw3)[0]),
        "rsv_merkle_hash_node": (lambda: rsv.hash_node((l8, r8), cols), ob.hash_node((l8, r8), cols)),
        "rsv_merkle_path_root": (lambda: rsv.merkle_path_root(q, sib, pcols, n_cols_at), ob.merkle_path_root(q, sib, pcols, n_cols_at)),
        "rsv_field_op": (lambda: rsv.field_op(rsv.F_QMUL, a4, b4), ob.field_op(rsv.F_QMUL, a4, b4)),
        "rsv_domain_points": (lambda: rsv.domain_points(13, dq), ob.domain_points(13, dq)),
        "rsv_line_eval": (lambda: rsv.line_eval(coeffs, xs), good),
        "rsv_last_layer_check": (lambda: rsv.last_layer_check(coeffs, xs, folded), (folded == good).all(axis=1).astype(np.uint8)),
        "rsv_oods_eval": (lambda: rsv.oods_eval(sm, pr), ob.oods_eval(sm, pr)),
    }


@pytest.mark.parametrize("n", [1, 257])
def test_every_probe_at_one_element_and_one_past_a_workgroup(rsv, n):
    for name, (call, want) in _probe_cases(rsv, n, 7 + n).items():
        got = call()
        assert np.array_equal(np.asarray(got).reshape(np.asarray(want).shape), want), name
    if n == 1:  # the eleventh: one proof
        proof = read_proof(SMALL)
        assert rsv.transcript(proof) == rsv._parse_transcript(ob.transcript_raw(proof))


def test_a_noncanonical_word_is_range_and_writes_nothing(rsv):
    """The probes with a bad flag (set by the kernel: the Poseidon2 ones and rsv_merkle_hash_node) and those that check
    their words on the host: RSV_E_RANGE, and the output buffer still holds the sentinel it was given."""
    n, lib = 257, rsv.lib
    z = lambda *s: np.zeros(s, np.uint32)

    def bad(*s):
        a = np.zeros(s, np.uint32)
        a.reshape(-1)[a.size - 3] = P  # in the last element: past the first workgroup
        return a
    p32 = lambda a: a.ctypes.data_as(rsv._u32p)
    outs = lambda *s: np.full(s, SENTINEL * 0x01010101, np.uint32)
    params = np.zeros((n, 26), np.uint32)
    params[:, :2] = 4
    bad_params = params.copy()
    bad_params[n - 1, 25] = P
    cases = {
        "rsv_poseidon2_permute": lambda o: lib.rsv_poseidon2_permute(p32(bad(n, 16)), p32(o), n, 0),
        "rsv_poseidon2_half_permute left": lambda o: lib.rsv_poseidon2_half_permute(p32(bad(n, 8)), p32(z(n, 8)), None, p32(o), None, n, 0),
        "rsv_poseidon2_half_permute right": lambda o: lib.rsv_poseidon2_half_permute(p32(z(n, 8)), p32(bad(n, 8)), None, None, p32(o), n, 0),
        "rsv_poseidon2_emulated": lambda o: lib.rsv_poseidon2_emulated(p32(z(n, 8)), p32(bad(n, 8)), None, p32(o), n, 0),
        "rsv_merkle_hash_node child": lambda o: lib.rsv_merkle_hash_node(p32(bad(n, 8)), p32(z(n, 8)), None, 0, p32(o), n, 0),
        "rsv_merkle_hash_node column": lambda o: lib.rsv_merkle_hash_node(None, None, p32(bad(n, 5)), 5, p32(o), n, 0),
        "rsv_field_op": lambda o: lib.rsv_field_op(rsv.F_QADD, p32(z(n, 4)), p32(bad(n, 4)), p32(o), n, 0),
        "rsv_line_eval": lambda o: lib.rsv_line_eval(p32(z(4, 4)), 2, p32(bad(n)), p32(o), n, 0),
        "rsv_last_layer_check": lambda o: lib.rsv_last_layer_check(p32(z(4, 4)), 2, p32(z(n)), p32(bad(n, 4)), o.ctypes.data_as(rsv._u8p), n, 0),
        "rsv_oods_eval sample": lambda o: lib.rsv_oods_eval(p32(bad(n, 142, 4)), p32(params), p32(o), n, 0),
        "rsv_oods_eval parameter": lambda o: lib.rsv_oods_eval(p32(z(n, 142, 4)), p32(bad_params), p32(o), n, 0),
    }
    for name, call in cases.items():
        o = outs(n, 416 * 4) if "emulated" in name else outs(n, 16)
        assert call(o) == RANGE and _untouched([o]), name
    # ... and the same process goes on to a correct call of a probe
    st = np.arange(16, dtype=np.uint32)[None]
    assert np.array_equal(rsv.poseidon2_permute(st), ob.poseidon2_permute(st))
