"""The builder with a proof's own public inputs, on the host (no device): tests/witness_inputs_host.cpp drives
circuit_program.hpp's build_program with hints recorded by the C oracle, and what it writes must be, word for word, the
oracle's circuit (oracle/recursion_circuit, as it is) with those inputs allocated PublicInput before anything else.

Templates.  The records come in the order (2, i), (3, j), (1, one) with n_fixed = 2: the own input is (1, one), the only M31
among the three standard inputs (a PublicInput row enforces M31).  The template for that is recursive_proof_16_15.bin,
the smallest fixture whose statement IS those three; small_proof.bin, the smallest fixture of all, verifies under (1, one)
alone (under the three the C oracle rejects it: RSV_R_LOGUP, asserted below) and is run with that one record as its own
input, n_fixed = 0.  Both give num_input = 4, and 5 with two copies (variables 4 and 5).
The stand-alone program is built twice, plainly and under AddressSanitizer + UBSan, and every case runs under both."""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import witness_inputs_ref as W
from tests.conftest import fixture_cfg, read_proof
from tests.test_recursion_circuit import _Sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
ONE, I, J = (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0)
THREE = [(2, I), (3, J), (1, ONE)]
WALKS = {0: ((0, -1), (0, -1)), 3: ((-1, 0), (-1, 0))}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp(request.param) / "witness_inputs_host")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "witness_inputs_host.cpp")])
    return exe


def _run(harness, *args):
    out = subprocess.run([harness, *args], capture_output=True, text=True, env=SAN_ENV, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    return out.stdout


def _built(harness, tmp_path, name, inputs, n_fixed, walks):
    hints, out_path = str(tmp_path / "hints.bin"), str(tmp_path / "program.bin")
    W.write_hints(hints, read_proof(name), inputs, len(walks), walks)
    _run(harness, "program", hints, str(n_fixed), out_path)
    return W.read_program(out_path)


def test_the_small_fixture_has_one_input_only():
    """Why the three-record template is recursive_proof_16_15.bin: small_proof.bin's statement is (1, one) alone."""
    small, cfg = read_proof("small_proof.bin"), fixture_cfg("small_proof.bin")
    assert [int(x[0]) for x in ob.verify_batch([small], cfg, [(1, ONE)])] == [1, 0]
    assert [int(x[0]) for x in ob.verify_batch([small], cfg, THREE)] == [0, 3]
    assert [int(x[0]) for x in ob.verify_batch([read_proof("recursive_proof_16_15.bin")], fixture_cfg("recursive_proof_16_15.bin"), THREE)] == [1, 0]


@pytest.mark.parametrize("name,inputs,n_fixed,walks", [
    ("recursive_proof_16_15.bin", THREE, 2, [0]),
    ("recursive_proof_16_15.bin", THREE, 2, [0, 3]),       # two copies, the second with both HashSet walks flipped
    ("small_proof.bin", [(1, ONE)], 0, [0]),
    ("small_proof.bin", [(1, ONE)], 0, [3, 0]),
])
def test_builder_writes_the_oracles_circuit_with_public_inputs(harness, tmp_path, name, inputs, n_fixed, walks):
    copies, n_own = len(walks), len(inputs) - n_fixed
    got = _built(harness, tmp_path, name, inputs, n_fixed, walks)
    proof = read_proof(name)
    c, d = W.build_circuit(proof, inputs, n_fixed, copies, [WALKS[w] for w in walks])
    ref = W.extract(c, d, copies, n_own)
    # n_vars, num_input, the gate list, the flow wires, the witness ops, the program: word for word
    assert got["n_vars"] == ref.n_vars == len(c.variables)
    assert got["num_input"] == c.num_input == 3 + copies == (4 if copies == 1 else 5)
    assert np.array_equal(got["gates"].astype(np.int64), W.gate_rows(c))
    assert np.array_equal(got["flow_wires"], ref.flow_wires)
    assert np.array_equal(got["instr"], ref.instr) and np.array_equal(got["levels"], ref.level_offsets)
    inputs_at = [int(r[1]) for r in got["instr"] if r[0] == W.W_INPUT]
    assert inputs_at == list(range(4, 4 + copies)) and got["copy_of"][4:4 + copies].tolist() == list(range(copies))
    for v in inputs_at:
        assert got["gates"][v].tolist() == [v, 0, v, 1, 0, 1] and tuple(c.variables[v]) == ONE
    # the rows whose op follows the witness, against the oracle's rows and values: (row, bit, constant) names a row (bit, 0,
    # c, op) whose c is bit * constant in the program and whose op is the constant where the template's bit is 1, else 0
    ops, by_dst = got["witness_ops"], got["instr"][np.argsort(got["instr"][:, 1])]
    rows = W.gate_rows(c)[ops[:, 0]]
    assert len(ops) and (rows[:, 0] == ops[:, 1]).all() and (rows[:, 1] == 0).all()
    assert (by_dst[rows[:, 2], 0] == 3).all() and (by_dst[rows[:, 2], 2] == ops[:, 1]).all() and (by_dst[rows[:, 2], 4] == ops[:, 2]).all()
    bits = np.array([c.variables[v][0] for v in ops[:, 1]])
    assert set(bits.tolist()) <= {0, 1} and (rows[:, 3] == np.where(bits == 1, ops[:, 2], 0)).all()
    # the program run over the template in Python integers == the oracle's `variables`
    flow = ob.poseidon_flow(proof, inputs)
    values = W.interpret(ref, _Sources(proof, d, flow), lambda dst, k: inputs[n_fixed + k][1])
    assert values == [tuple(v) for v in c.variables]
    assert [values[v] for v in inputs_at] == [ONE] * copies


@pytest.mark.parametrize("name,inputs,walks", [("recursive_proof_16_15.bin", THREE, [0]), ("small_proof.bin", [(1, ONE)], [0, 3])])
def test_every_record_fixed_is_the_program_without_own_inputs(harness, tmp_path, name, inputs, walks):
    """n_fixed = n_pi: the arrays are the ones the argument list without n_fixed gives (compared inside the stand-alone
    program, array by array) and the oracle's circuit with every input a constant."""
    from oracle import recursion_circuit as rc
    got = _built(harness, tmp_path, name, inputs, len(inputs), walks)
    orders = [WALKS[w] for w in walks]
    c, d, _ = rc.build_circuit(read_proof(name), ob, inputs, multipliers=len(walks), shift_order=orders if len(walks) > 1 else orders[0])
    ref = rc.program.extract(c, d, len(walks))
    assert got["num_input"] == 3 and not (got["instr"][:, 0] == W.W_INPUT).any()
    assert got["n_vars"] == ref.n_vars and np.array_equal(got["instr"], ref.instr) and np.array_equal(got["levels"], ref.level_offsets)
    assert np.array_equal(got["flow_wires"], ref.flow_wires) and np.array_equal(got["gates"].astype(np.int64), W.gate_rows(c))


def test_refusals(harness):
    """check_program refuses W_INPUT with imm0 >= 4096 (and takes 4095); check_copies refuses a hint in another copy's
    range, a hint range that crosses copies, and an input variable out of its place."""
    assert "refusals: ok" in _run(harness, "refusals")


def test_the_library_exports_the_new_entry_points(rsv):
    """No device needed: the symbols, and the refusals that come before any device work."""
    import ctypes
    lib = rsv.lib
    for name in ("rsv_witness_program_build_inputs", "rsv_witness_program_inputs", "rsv_witness_eval_inputs_dev", "rsv_witness_eval_inputs",
                 "rsv_witness_eval_groups_inputs_dev"):
        assert hasattr(lib, name), name
    assert lib.rsv_witness_program_inputs(None, None, None, None) == -1                                        # RSV_E_NULL
    assert lib.rsv_witness_eval_inputs_dev(None, None, None, None, 1, None, None, 0, None, 0, None, None, None, None, None) == -1
    assert lib.rsv_witness_eval_groups_inputs_dev(None, None, None, None, 1, None, None, 0, None, 0, None, None, None, None, None, None) == -1
    assert lib.rsv_witness_program_build_inputs(None, 0, None, None, 0, 0, 1, None, 0, None) == -1
    proof, cfg, h = np.zeros(64, np.uint8), rsv.PcsConfig(3, 1, 0, 9), ctypes.c_void_p()
    args = (proof.ctypes.data_as(rsv._u8p), 64, ctypes.byref(cfg), rsv.make_inputs([(1, ONE)]), 1)
    assert lib.rsv_witness_program_build_inputs(*args, 2, 1, None, 0, ctypes.byref(h)) == -2                    # n_fixed > n_pi: RSV_E_SIZE
    assert lib.rsv_witness_program_build_inputs(*args, 0, 0, None, 0, ctypes.byref(h)) == -2                    # no copies
