"""The hashed statement on the host (no device): the digest's definition against the oracle's gadget, and the builder of a
hashed program — tests/statement_host.cpp drives circuit_program.hpp's build_program with hints recorded by the C oracle,
and what it writes must be, word for word, the oracle's circuit (oracle/recursion_circuit, as it is) with the layout of
tests/statement_ref.py: the statement, the own records, the hash that ties them, the copies.

The template is recursive_proof_16_15.bin with the records in the order (2, i), (3, j), (1, one) and n_fixed = 2: its own
record is (1, one), the only M31 among the three, and it is the smallest fixture that verifies under the three
(tests/test_witness_inputs_host.py).  The stand-alone program is built twice, plainly and under AddressSanitizer + UBSan,
and every case runs under both; it is never loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import statement_ref as S
from tests import witness_inputs_ref as W
from tests.conftest import read_proof
from tests.test_recursion_circuit import _Sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
ONE, I, J = (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0)
THREE = [(2, I), (3, J), (1, ONE)]
WALKS = {0: ((0, -1), (0, -1)), 3: ((-1, 0), (-1, 0))}
NAME = "recursive_proof_16_15.bin"


@pytest.mark.parametrize("T", S.T_CASES)
def test_the_digest_is_the_oracles_gadget_and_hash_node(T):
    """hash_m31_columns_get_rate of T words: the circuit gadget's value, the restated sponge and hash_node(None, v) agree;
    the gadget invokes the permutation ceil(T / 8) + 1 times with the states of the restatement, swap 0 in all."""
    v = np.random.default_rng(T).integers(0, S.P, T)
    want = ob.hash_node(None, v.astype(np.uint32))[0].tolist()
    got, c = S.gadget_digest(v)
    states = S.sponge_states(v)
    assert got == want == S.digest(v) and len(c.flow) == len(states) == -(-T // 8) + 1
    for (e1, e2, e3, e4, _addr, swap), (left, right, out) in zip(c.flow, states):
        assert not swap and list(e1[1]) == left and list(e2[1]) == right and list(e3[1]) + list(e4[1]) == out
    c.check_arithmetics()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp(request.param) / "statement_host")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "statement_host.cpp")])
    return exe


def _run(harness, *args):
    out = subprocess.run([harness, *args], capture_output=True, text=True, env=SAN_ENV, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    return out.stdout


@pytest.mark.parametrize("walks", [[0], [0, 3]])
def test_builder_writes_the_oracles_hashed_circuit(harness, tmp_path, walks):
    copies, n_fixed, n_own = len(walks), 2, 1
    proof = read_proof(NAME)
    words = [1] * copies                                       # the own record (1, one), once per copy
    hints, stmt_path, out_path = str(tmp_path / "hints.bin"), str(tmp_path / "stmt.bin"), str(tmp_path / "program.bin")
    W.write_hints(hints, proof, THREE, copies, walks)
    S.flow_records(words).tofile(stmt_path)
    _run(harness, "program", hints, str(n_fixed), stmt_path, out_path)
    got = W.read_program(out_path)
    c, d = S.build_circuit(proof, THREE, n_fixed, copies, [WALKS[w] for w in walks])
    ref, F, n_hash = S.extract(c, d, copies, n_own)
    # n_vars, num_input, the gate list, the flow wires, the program: word for word
    assert got["n_vars"] == ref.n_vars == len(c.variables) and n_hash == 2
    assert got["num_input"] == c.num_input == 11
    assert np.array_equal(got["gates"].astype(np.int64), W.gate_rows(c))
    assert np.array_equal(got["flow_wires"], ref.flow_wires) and len(ref.flow_wires) == copies * F + n_hash
    assert np.array_equal(got["instr"], ref.instr) and np.array_equal(got["levels"], ref.level_offsets)
    by_dst = got["instr"][np.argsort(got["instr"][:, 1])]
    assert by_dst[4:12, 0].tolist() == [S.W_STMT] * 8 and by_dst[4:12, 4].tolist() == list(range(8))
    assert by_dst[12:12 + copies, 0].tolist() == [S.W_INPUT] * copies and got["copy_of"][12:12 + copies].tolist() == list(range(copies))
    assert (got["instr"][:, 0] == S.W_INPUT).sum() == copies and (got["instr"][:, 0] == S.W_STMT).sum() == 8
    for v in range(4, 12 + copies):
        assert got["gates"][v].tolist() == [v, 0, v, 1, 0, 1]
    assert [c.variables[4 + k][0] for k in range(8)] == S.digest(words) and all(tuple(c.variables[12 + k]) == ONE for k in range(copies))
    # the program run over the template in Python integers == the oracle's `variables`
    flow = ob.poseidon_flow(proof, THREE)
    tail = np.concatenate([S.flow_records(words), np.zeros((n_hash, 1), np.uint32)], axis=1)
    assert flow.shape == (F, 33)
    values = S.interpret(ref, _Sources(proof, d, np.concatenate([flow] * copies + [tail])), lambda dst, k: THREE[n_fixed + k][1], S.digest(words))
    assert values == [tuple(v) for v in c.variables]
    c.check_arithmetics()


def test_refusals(harness):
    """build_program refuses a hashed program without own inputs; check_program refuses W_STMT with imm0 >= 8 and a W_FLOW
    beyond the tail; check_copies refuses every misplacement of the statement, the inputs and the hash."""
    assert "refusals: ok" in _run(harness, "refusals")


def test_the_library_exports_the_new_entry_points(rsv):
    """No device needed: the symbols, the option, and the refusals that come before any device work."""
    import ctypes
    lib = rsv.lib
    for name in ("rsv_statement_digest_dev", "rsv_witness_program_build_inputs_hashed", "rsv_witness_program_statement"):
        assert hasattr(lib, name), name
    assert lib.rsv_statement_digest_dev(None, None, 1, 1, 1, None, None) == -1                                  # RSV_E_NULL
    assert lib.rsv_witness_program_statement(None, None, None, None) == -1
    assert lib.rsv_witness_program_build_inputs_hashed(None, 0, None, None, 0, 0, 1, None, 0, None) == -1
    proof, cfg, h = np.zeros(64, np.uint8), rsv.PcsConfig(3, 1, 0, 9), ctypes.c_void_p()
    args = (proof.ctypes.data_as(rsv._u8p), 64, ctypes.byref(cfg), rsv.make_inputs([(1, ONE)]), 1)
    assert lib.rsv_witness_program_build_inputs_hashed(*args, 1, 1, None, 0, ctypes.byref(h)) == -2              # no own input: RSV_E_SIZE
    assert lib.rsv_witness_program_build_inputs_hashed(*args, 2, 1, None, 0, ctypes.byref(h)) == -2
    assert lib.rsv_witness_program_build_inputs_hashed(*args, 0, 0, None, 0, ctypes.byref(h)) == -2              # no copies
    opt = rsv.OPTIONS["statement_row_max"]
    assert opt == 31
    for value, want in ((-1, -5), ((1 << 26) + 2, -5), ((1 << 26) + 1, 0), (1, 0), (0, 0)):
        assert lib.rsv_ctx_set_option(None, opt, value) == want, value
