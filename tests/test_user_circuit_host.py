"""A caller's own circuit as the chain's program, without a device: rsv_circuit_program_create and its refusals,
rsv_trace_preprocessed_inputs against the oracle's columns for the three circuits of tests/user_circuit_ref.py, the numpy
model of the two device checks against the oracle's check_arithmetics / check_poseidon_invocations, and
recursive-stwo_amd/csrc/user_circuit_host.hpp under AddressSanitizer + UBSan (tests/user_circuit_host_asan.cpp, a program
of its own run as a child process)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import user_circuit_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
NULL, SIZE, RANGE = -1, -2, -5
_BUILT = {}


def built(kind):
    if kind not in _BUILT:
        _BUILT[kind] = U.build(kind)
    return _BUILT[kind]


def _pre(rsv, fn, gates, wires, lp, lq, *num_input):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    plonk, poseidon = np.zeros((10, 1 << lp), np.uint32), np.zeros((40, 1 << lq), np.uint32)
    rc = fn(gates.ctypes.data_as(u32p), len(gates), wires.ctypes.data_as(u32p), len(wires), lp, lq, *num_input, plonk.ctypes.data_as(u32p),
            poseidon.ctypes.data_as(u32p))
    return rc, plonk, poseidon


def test_three_inputs_is_rsv_trace_preprocessed(rsv):
    """S1 with its public input a plain witness: rsv_trace_preprocessed_inputs(num_input = 3) == rsv_trace_preprocessed."""
    b = U.build("S1", public=False)
    assert b.num_input == 3
    lp, lq = rsv.trace_log_sizes(len(b.gates), len(b.flow_wires))
    rc0, p0, q0 = _pre(rsv, rsv.lib.rsv_trace_preprocessed, b.gates, b.flow_wires, lp, lq)
    rc1, p1, q1 = _pre(rsv, rsv.lib.rsv_trace_preprocessed_inputs, b.gates, b.flow_wires, lp, lq, 3)
    assert rc0 == 0 and rc1 == 0 and p0.tobytes() == p1.tobytes() and q0.tobytes() == q1.tobytes()
    ppre, _, qpre, _, _, _ = U.columns(b)
    assert np.array_equal(p1, ppre) and np.array_equal(q1, qpre)
    assert _pre(rsv, rsv.lib.rsv_trace_preprocessed_inputs, b.gates, b.flow_wires, lp, lq, 2)[0] == RANGE


@pytest.mark.parametrize("kind", U.KINDS)
def test_preprocessed_columns_with_a_public_input(rsv, kind):
    """All 10 + 40 columns == the oracle's (pad, populate_logup_arguments with num_input = 4, the Poseidon AIR's rows), and
    the shapes are the ones the circuits are there for."""
    b = built(kind)
    ppre, _, qpre, _, lp, lq = U.columns(b)
    assert b.num_input == 4 and rsv.trace_log_sizes(len(b.gates), len(b.flow_wires)) == (lp, lq)
    assert {"S1": lp <= 7 and lq == 8, "S2": (lp, lq) == (12, 8), "S3": lq == 9 and len(b.flow_wires) == 33}[kind]
    plonk, poseidon = rsv.trace_preprocessed(b.gates, b.flow_wires, num_input=4)
    for k, name in enumerate(U.T.PREPROCESSED):
        assert np.array_equal(plonk[k], ppre[k]), name
    assert np.array_equal(poseidon, qpre), [k for k in range(40) if not np.array_equal(poseidon[k], qpre[k])]
    three = rsv.trace_preprocessed(b.gates, b.flow_wires)[0]
    assert not np.array_equal(three, plonk)   # the input's multiplicity is what num_input changes
    c = rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, b.witness_ops)
    got = c.preprocessed()
    assert np.array_equal(got[0], ppre) and np.array_equal(got[1], qpre) and c.trace_sizes() == (lp, lq)
    c.close()


def _create(rsv, gates, wires, ops, n_vars, num_input, null=()):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    arr = {"gates": np.ascontiguousarray(gates, np.uint32), "wires": np.ascontiguousarray(wires, np.uint32), "ops": np.ascontiguousarray(ops, np.uint32)}
    ptr = {k: None if k in null else a.ctypes.data_as(u32p) for k, a in arr.items()}
    h = ctypes.c_void_p()
    rc = rsv.lib.rsv_circuit_program_create(ptr["gates"], len(arr["gates"]), ptr["wires"], len(arr["wires"]), ptr["ops"], len(arr["ops"]), n_vars,
                                            num_input, 0, None if "out" in null else ctypes.byref(h))
    if rc == 0:
        rsv.lib.rsv_witness_program_destroy(h)
    else:
        assert not h.value
    return rc


def test_create_gives_back_what_went_in_and_refuses_the_rest(rsv):
    b = built("S1")
    c = rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, b.witness_ops)
    gates, ops = c.gates()
    assert np.array_equal(gates, b.gates) and np.array_equal(ops, b.witness_ops)
    prog = c.export()
    assert np.array_equal(prog.flow_wires, b.flow_wires) and len(prog.instr) == 0 and prog.level_offsets.tolist() == [0]
    s = c.shape
    assert (c.n_vars, c.n_levels, c.num_input, s.copies, s.flow_count) == (b.n_vars, 0, 4, 1, len(b.flow_wires))
    assert (s.log_size_plonk, s.log_size_poseidon, s.pow_bits, s.log_blowup, s.log_last, s.n_queries, s.n_inner) == (0,) * 7
    c.close()
    no_ops = rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input)   # witness_ops NULL with a count of 0
    assert len(no_ops.gates()[1]) == 0
    no_ops.close()

    g, w, o, nv, ni = b.gates, b.flow_wires, b.witness_ops, b.n_vars, b.num_input
    assert _create(rsv, g, w, o, nv, ni) == 0
    for name in ("gates", "wires", "ops", "out"):
        assert _create(rsv, g, w, o, nv, ni, null=(name,)) == NULL, name
    assert _create(rsv, g[:0], w, o[:0], nv, ni) == SIZE                 # zero rows
    assert _create(rsv, g, w[:0], o, nv, ni) == SIZE                     # zero flow
    assert _create(rsv, g, w, o, (1 << 26) + 1, ni) == SIZE              # n_vars beyond the bound
    assert _create(rsv, g, w, o, nv - 1, ni) == RANGE                    # the last variable's wires are out of range

    def changed(arr, at, value):
        a = arr.copy()
        a[at] = value
        return a
    assert _create(rsv, changed(g, (10, 1), nv), w, o, nv, ni) == RANGE  # a wire
    assert _create(rsv, g, w, changed(o, (0, 1), nv), nv, ni) == RANGE   # a bit variable
    assert _create(rsv, g, changed(w, (2, 4), nv), o, nv, ni) == RANGE   # a swap address
    assert _create(rsv, changed(g, (3, 3), 0), w, o, nv, ni) == RANGE    # the constant rows
    assert _create(rsv, g[1:], w, o, nv, ni) == RANGE
    assert _create(rsv, g, w, o, nv, 2) == RANGE and _create(rsv, g, w, o, nv, nv) == RANGE
    pw = int(w[0, 0])
    row = int(np.flatnonzero(g[:, 4] == pw)[0])
    assert pw and _create(rsv, changed(g, (row, 4), 0), w, o, nv, ni) == RANGE        # a flow wire no row carries
    other = int(np.flatnonzero((g[:, 4] != 0) & (g[:, 4] != pw))[0])
    assert _create(rsv, changed(g, (other, 4), pw), changed(w, np.nonzero(w == g[other, 4]), 0), o, nv, ni) == RANGE  # two rows carry it
    twice = np.concatenate([g, np.array([[pw, 0, pw, 1, 0, 0]], np.uint32)])
    assert _create(rsv, twice, w, o, nv, ni) == RANGE                    # a Poseidon wire used more than once
    with pytest.raises(rsv.RsvError) as e:
        rsv.Circuit(twice, w, nv, ni, o)
    assert e.value.code == RANGE


def test_witness_entry_points_refuse_a_created_program(rsv):
    """Before any device work: the statuses show without a device."""
    b = built("S1")
    c = rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, b.witness_ops)
    lib, h, out = rsv.lib, c._h, ctypes.c_size_t(0)
    assert lib.rsv_witness_scratch_bytes(h, 1, ctypes.byref(out)) == SIZE
    assert lib.rsv_witness_group_scratch_bytes(h, 1, ctypes.byref(out)) == SIZE
    blob, offsets = rsv.pack([b"\0" * 64])
    u8p, u64p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    cfg = rsv.prepare_cfg(rsv.PcsConfig(20, 5, 8, 16), 1)
    pi = rsv.make_inputs(b.inputs)
    lead = (h, blob.ctypes.data_as(u8p), offsets.ctypes.data_as(u64p), 1, cfg.ref(), pi, len(b.inputs))
    variables, acc, reason = np.zeros((1, b.n_vars, 4), np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    a8, r8 = acc.ctypes.data_as(u8p), reason.ctypes.data_as(u8p)
    big = np.zeros(1 << 16, np.uint32).ctypes.data_as(u32p)
    assert lib.rsv_witness_eval(*lead, variables.ctypes.data_as(u32p), None, None, a8, r8, 0) == SIZE
    assert lib.rsv_witness_trace(*lead, big, big, big, a8, r8, 0) == SIZE
    assert lib.rsv_witness_interaction(*lead, big, big, big, big, a8, a8, r8, 0) == SIZE
    assert lib.rsv_witness_commit(*lead, 1, big, big, big, a8, a8, r8, 0) == SIZE
    one = ctypes.c_void_p(16)   # non-NULL, 16-byte aligned, never dereferenced: the refusal comes first
    assert lib.rsv_witness_eval_dev(one, h, one, one, 1, cfg.ref(), pi, len(b.inputs), one, None, None, one, None) == SIZE
    assert lib.rsv_witness_eval_groups_dev(one, h, one, one, 1, cfg.ref(), pi, len(b.inputs), one, None, None, one, one, None) == SIZE
    c.close()


@pytest.mark.parametrize("kind", U.KINDS)
def test_model_is_the_oracles_checks(kind):
    """The numpy model accepts what cs.check_arithmetics / cs.check_poseidon_invocations accept, and names the row or
    invocation at which the oracle's assert fires on tampered copies."""
    b = built(kind)
    b.cs.check_arithmetics()
    b.cs.check_poseidon_invocations(U.permute)
    assert U.model_check(b.gates, b.witness_ops, b.variables) == U.NONE
    bad, flow, swap = U.model_flow(b.gates, b.flow_wires, b.variables, b.unbound_flow())
    assert bad == U.NONE and np.array_equal(flow, b.flow) and np.array_equal(swap, b.swap)

    def oracle_row(variables):
        saved = b.cs.variables
        b.cs.variables = [tuple(int(x) for x in v) for v in variables]
        try:
            b.cs.check_arithmetics()
            return U.NONE
        except AssertionError as e:
            return e.args[0] if isinstance(e.args[0], int) else e.args[0][0]
        finally:
            b.cs.variables = saved

    rnd = np.random.default_rng(7)
    for var in [4, b.n_vars - 1] + [int(x) for x in rnd.integers(4, b.n_vars, 6)]:
        v = b.variables.copy()
        v[var, 0] = (v[var, 0] + 1) % U.P
        want = oracle_row(v)
        assert want != U.NONE and U.model_check(b.gates, b.witness_ops, v) == want, var

    # a bound output changed: the oracle's check_poseidon_invocations fails, the model at the invocation that binds it
    k = int(np.flatnonzero(b.flow_wires[:, 2] != 0)[-1])
    row = int(np.flatnonzero(b.gates[:, 4] == b.flow_wires[k, 2])[0])
    v = b.variables.copy()
    v[b.gates[row, 0], 1] ^= 1
    first = min(j for j in range(len(b.flow_wires)) if b.flow_wires[k, 2] in b.flow_wires[j, :4])
    assert U.model_flow(b.gates, b.flow_wires, v, b.unbound_flow())[0] == first
    saved, b.cs.variables = b.cs.variables, [tuple(int(x) for x in r) for r in v]
    try:
        with pytest.raises(AssertionError):
            b.cs.check_poseidon_invocations(U.permute)
    finally:
        b.cs.variables = saved


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("asan") / "user_circuit_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "user_circuit_host_asan.cpp")])
    return exe


def _clean(out, word):
    assert out.returncode == 0 and word in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_validation_header_under_sanitizers(harness, tmp_path):
    _clean(subprocess.run([harness, "adversarial"], capture_output=True, text=True, env=SAN_ENV, timeout=600), "adversarial ok")
    for kind in ("S1", "S3"):
        b = built(kind)
        path = str(tmp_path / f"{kind}.bin")
        hdr = np.array([0x55435631, len(b.gates), len(b.flow_wires), len(b.witness_ops), b.n_vars, b.num_input], np.uint32)
        np.concatenate([hdr, b.gates.reshape(-1), b.flow_wires.reshape(-1), b.witness_ops.reshape(-1)]).tofile(path)
        _clean(subprocess.run([harness, "file", path, "5", "400"], capture_output=True, text=True, env=SAN_ENV, timeout=600), "recorded ok")
