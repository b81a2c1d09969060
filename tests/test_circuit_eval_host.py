"""A caller's circuit compiled into an evaluation program, without a device: rsv_circuit_program_create_eval and its
refusals, the structure of the exported program for the four circuits of tests/circuit_eval_ref.py, the exported program
run by a Python-integer interpreter against the oracle's own variables, flow and swap bits (which pins the definition rule
of include/rsv.h), and recursive-stwo_amd/csrc/circuit_eval_host.hpp under AddressSanitizer + UBSan
(tests/circuit_eval_host_asan.cpp, a program of its own run as a child process)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import circuit_eval_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
NULL, SIZE, RANGE = -1, -2, -5
_BUILT = {}


def built(kind, seed=1, bit=1):
    key = (kind, seed, bit)
    if key not in _BUILT:
        _BUILT[key] = E.build(kind, pub=(11 + 7 * seed, 0, 0, 0), seed=seed, bit=bit)
    return _BUILT[key]


def _circuit(rsv, b):
    return rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, **E.create_args(b))


def _create(rsv, b, hints=None, links=None, n_inputs=None, gates=None, n_vars=None, null=()):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    a = E.create_args(b)
    arr = {"gates": b.gates if gates is None else gates, "wires": b.flow_wires, "ops": b.witness_ops,
           "hints": a["hints"] if hints is None else hints, "links": a["flow_links"] if links is None else links}
    arr = {k: np.ascontiguousarray(x, np.uint32) for k, x in arr.items()}
    ptr = {k: None if k in null else x.ctypes.data_as(u32p) for k, x in arr.items()}
    h = ctypes.c_void_p()
    rc = rsv.lib.rsv_circuit_program_create_eval(ptr["gates"], len(arr["gates"]), ptr["wires"], len(arr["wires"]), ptr["ops"], len(arr["ops"]),
                                                 b.n_vars if n_vars is None else n_vars, b.num_input, ptr["hints"], len(arr["hints"]), ptr["links"],
                                                 a["n_inputs"] if n_inputs is None else n_inputs, 0, None if "out" in null else ctypes.byref(h))
    if rc == 0:
        rsv.lib.rsv_witness_program_destroy(h)
    else:
        assert not h.value   # *out is untouched
    return rc


def test_refusals_leave_out_untouched(rsv):
    b = built("S1")
    a = E.create_args(b)
    hints, links, nv = a["hints"], a["flow_links"], b.n_vars
    assert _create(rsv, b) == 0 and _create(rsv, b, null=("links",)) == 0       # NULL links: every half without a wire is read from d_flow

    def hint(at, col, value):
        h = hints.copy()
        h[at, col] = value
        return h
    inputs = np.flatnonzero(hints[:, 1] == E.INPUT)
    i0, i1 = int(inputs[0]), int(inputs[1])
    # rsv_circuit_program_create's own refusals come first, with its statuses
    assert _create(rsv, b, null=("out",)) == NULL and _create(rsv, b, null=("gates",)) == NULL
    assert _create(rsv, b, gates=b.gates[:0]) == SIZE
    assert _create(rsv, b, n_vars=nv - 1) == RANGE
    assert _create(rsv, b, null=("hints",)) == NULL                              # NULL hints with a count
    assert _create(rsv, b, n_inputs=(1 << 26) + 1) == SIZE
    for what, h in (("dst", hint(i0, 0, nv)), ("kind", hint(i0, 1, 8)), ("slot", hint(i0, 3, a["n_inputs"])),
                    ("src", np.concatenate([hints[:i0], [[hints[i0, 0], E.COPY, nv, 0]], hints[i0 + 1:]])),
                    ("cinv imm", np.concatenate([hints[:i0], [[hints[i0, 0], E.CINV, 1, 2]], hints[i0 + 1:]])),
                    ("coord imm", np.concatenate([hints[:i0], [[hints[i0, 0], E.COORD, 1, 4]], hints[i0 + 1:]])),
                    ("bit imm", np.concatenate([hints[:i0], [[hints[i0, 0], E.BIT, 1, 32]], hints[i0 + 1:]])),
                    ("two hints for one dst", np.concatenate([hints, hints[i0:i0 + 1]])),
                    ("a hint on a constant", np.concatenate([hints, [[2, E.COPY, 1, 0]]])),
                    ("no definition", np.delete(hints, i0, axis=0)),
                    ("a cycle", np.concatenate([np.delete(hints, [i0, i1], axis=0), [[hints[i0, 0], E.COPY, hints[i1, 0], 0]],
                                                [[hints[i1, 0], E.COPY, hints[i0, 0], 0]]]))):
        assert _create(rsv, b, hints=h) == RANGE, what
    assert _create(rsv, b, hints=hints[:0]) == RANGE                             # empty hints: S1's inputs have no definition
    wired = np.argwhere(b.flow_wires[:, :2] != 0)[0]
    free = np.argwhere((b.flow_wires[:, :2] == 0) & (links == 0))[0]
    for what, at, value in (("a link on a half with a wire", wired, 1), ("k' >= n_flow", free, 1 + 2 * len(links)),
                            ("k' == k", free, 1 + 2 * int(free[0]))):
        l = links.copy()
        l[at[0], at[1]] = value
        assert _create(rsv, b, links=l) == RANGE, what
    # a chain of links that closes: S4's sponge starts at an invocation with a free half; let that half read the chain's end
    s4 = built("S4")
    l4 = E.links_of(s4.cs)
    start = int(np.flatnonzero((s4.flow_wires[:, 1] == 0) & (l4[:, 1] == 0))[0])
    end = int(np.flatnonzero((l4 != 0).all(axis=1))[-1])
    assert end > start and _create(rsv, s4) == 0
    l4[start, 1] = 1 + 2 * end
    assert _create(rsv, s4, links=l4) == RANGE
    # an output wire two invocations name: the variables of its row would have two definitions
    two = b.flow_wires.copy()
    ks = np.flatnonzero(two[:, 2] != 0)
    two[ks[1], 2] = two[ks[0], 2]
    arr = E.create_args(b)
    h = ctypes.c_void_p()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    p = lambda x: np.ascontiguousarray(x, np.uint32).ctypes.data_as(u32p)
    assert rsv.lib.rsv_circuit_program_create_eval(p(b.gates), len(b.gates), p(two), len(two), p(b.witness_ops), len(b.witness_ops), nv, b.num_input,
                                                   p(arr["hints"]), len(arr["hints"]), p(links), arr["n_inputs"], 0, ctypes.byref(h)) == RANGE
    assert not h.value


def test_info_and_export_need_an_evaluation_program(rsv):
    b = built("S1")
    plain = rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, b.witness_ops)
    with pytest.raises(rsv.RsvError) as e:
        plain.eval_info()
    assert e.value.code == SIZE
    out = ctypes.c_size_t(5)
    assert rsv.lib.rsv_circuit_eval_export(plain._h, None, None, None, None) == SIZE
    assert rsv.lib.rsv_circuit_eval_scratch_bytes(plain._h, 1, ctypes.byref(out)) == SIZE and out.value == 5
    one = ctypes.c_void_p(16)   # non-NULL, 16-byte aligned, never dereferenced: the refusal comes first
    assert rsv.lib.rsv_circuit_eval_dev(one, plain._h, one, 1, one, one, one, one, one) == SIZE
    c = _circuit(rsv, b)
    assert rsv.lib.rsv_circuit_eval_dev(one, c._h, one, 1, None, one, one, one, one) == NULL
    assert rsv.lib.rsv_circuit_eval_dev(one, c._h, one, 1, ctypes.c_void_p(8), one, one, one, one) == SIZE
    assert rsv.lib.rsv_circuit_eval_info(None, None, None, None) == NULL
    n_inputs, n_levels, n_instr = c.eval_info()
    assert n_inputs == len(E.inputs_of(b)) and n_levels > 1 and c.eval_scratch_bytes(70) == 0
    # everything rsv_circuit_program_create makes is there, and the verifier-witness entry points still refuse it
    gates, ops = c.gates()
    assert np.array_equal(gates, b.gates) and np.array_equal(ops, b.witness_ops) and c.n_levels == 0
    assert rsv.lib.rsv_witness_scratch_bytes(c._h, 1, ctypes.byref(out)) == SIZE
    plain.close()
    c.close()


@pytest.mark.parametrize("kind", E.KINDS)
def test_exported_program_structure(rsv, kind):
    """Every variable is defined exactly once (by an instruction, or as the output of one invocation), every operand and
    every invocation input sits at a strictly lower level than its user, flow_order is a permutation."""
    b = built(kind)
    c = _circuit(rsv, b)
    instr, levels, order, flevels = c.eval_export()
    n_inputs, n_levels, n_instr = c.eval_info()
    c.close()
    n_flow, links = len(b.flow_wires), E.links_of(b.cs)
    assert len(levels) == n_levels + 1 == len(flevels) and levels[0] == 0 == flevels[0] and levels[-1] == n_instr and flevels[-1] == n_flow
    assert (np.diff(levels.astype(np.int64)) >= 0).all() and (np.diff(flevels.astype(np.int64)) >= 0).all()
    assert sorted(order.tolist()) == list(range(n_flow))
    level_of_instr = np.repeat(np.arange(n_levels), np.diff(levels))
    level_of_flow = np.zeros(n_flow, np.int64)
    level_of_flow[order] = np.repeat(np.arange(n_levels), np.diff(flevels))
    var_level = np.full(b.n_vars, -1, np.int64)
    assert len(set(instr[:, 1].tolist())) == n_instr
    var_level[instr[:, 1]] = level_of_instr
    src = E.flow_sources(b.gates, b.flow_wires)
    for k in range(n_flow):
        for var in src[k, 2:].reshape(-1):
            if var >= 4 and var_level[var] < 0:
                var_level[var] = level_of_flow[k]
            else:
                assert var < 4 or var in instr[:, 1], (k, var)    # not defined twice
    assert (var_level >= 0).all()
    defined_by_flow = b.n_vars - n_instr
    assert defined_by_flow == sum(1 for o in b.cs.origin if o[0] == "hint" and o[1] is not None and o[1][0] == "perm")
    for (op, dst, x, y, i0, i1, i2, _), l in zip(instr.tolist(), level_of_instr.tolist()):
        reads = {0: [], 1: [x, y], 2: [x, y], E.E_INPUT: [], E.E_GATE: [x, y] + ([i1] if i2 else [])}.get(op, [x])
        assert all(var_level[r] < l for r in reads), (op, dst, reads)
    for k in range(n_flow):
        reads = [int(v) for h in range(2) if b.flow_wires[k, h] for v in src[k, h]] + ([int(b.flow_wires[k, 4])] if b.flow_wires[k, 4] else [])
        assert all(var_level[r] < level_of_flow[k] for r in reads), k
        assert all(level_of_flow[(int(l) - 1) // 2] < level_of_flow[k] for l in links[k] if l), k
    if kind == "S4":
        kinds = set(E.hints_of(b.cs)[:, 1].tolist())
        assert kinds == set(range(8)) and np.diff(flevels).max() >= 8 and (links != 0).all(axis=1).sum() >= 20
        assert E.E_GATE in instr[:, 0] and n_levels >= 24


@pytest.mark.parametrize("kind", E.KINDS)
def test_exported_program_reproduces_the_oracle(rsv, kind):
    """model_eval of the exported program on the inputs alone == the oracle's variables, flow and swap, word for word: two
    seeds, both values of the witness bit."""
    for seed, bit in ((1, 1), (2, 0), (1, 0), (2, 1)):
        b = built(kind, seed, bit)
        c = _circuit(rsv, b)
        exported = c.eval_export()
        c.close()
        tables = (b.gates, b.flow_wires, E.links_of(b.cs), b.n_vars)
        variables, flow, swap = E.model_eval(*exported, tables, E.inputs_of(b), E.flow_in_of(b))
        assert np.array_equal(variables, b.variables), np.flatnonzero((variables != b.variables).any(axis=1))[:8]
        assert np.array_equal(flow, b.flow) and np.array_equal(swap, b.swap)
    # the program does not depend on the witness: the same arrays for every seed and bit
    assert np.array_equal(E.hints_of(built(kind, 1, 1).cs), E.hints_of(built(kind, 2, 0).cs))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("asan") / "circuit_eval_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "circuit_eval_host_asan.cpp")])
    return exe


def _clean(out, word):
    assert out.returncode == 0 and word in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_compile_header_under_sanitizers(harness, tmp_path):
    _clean(subprocess.run([harness, "adversarial"], capture_output=True, text=True, env=SAN_ENV, timeout=600), "adversarial ok")
    for kind in E.KINDS:
        b = built(kind)
        a = E.create_args(b)
        path = str(tmp_path / f"{kind}.bin")
        hdr = np.array([0x43455631, len(b.gates), len(b.flow_wires), len(b.witness_ops), b.n_vars, b.num_input, len(a["hints"]), a["n_inputs"]], np.uint32)
        np.concatenate([hdr, b.gates.reshape(-1), b.flow_wires.reshape(-1), b.witness_ops.reshape(-1), a["hints"].reshape(-1),
                        a["flow_links"].reshape(-1)]).tofile(path)
        _clean(subprocess.run([harness, "file", path, "5", "300"], capture_output=True, text=True, env=SAN_ENV, timeout=600), "recorded ok")
