"""What the tests of per-proof public inputs in the recursion circuit share (no test lives here): the oracle's circuit with
a proof's own inputs allocated PublicInput (oracle/recursion_circuit, used as it is), the witness program of such a run
with its W_INPUT instructions, a Python-integer interpretation of it, and the hints file of tests/host_logic_asan.cpp.

The layout (include/rsv.h, rsv_witness_program_build_inputs): of the records `inputs`, the first n_fixed are constants of
the circuit and the others are the proof's own; record k of the proof that copy c verifies is variable 4 + c * n_own + k,
allocated before anything else, with the instruction (W_INPUT, imm0 = k)."""
import numpy as np

from oracle import recursion_circuit as rc
from oracle.recursion_circuit import cs as C
from oracle.recursion_circuit import gadgets, verifier
from tests import oracle_binding as ob

W_INPUT = 19          # layout.hpp: behind W_FRI_COL (18), so that no earlier op moved
MAX_OWN_INPUTS = 4096
P = C.P


def _permute(state):
    return ob.poseidon2_permute(np.array(state, dtype=np.uint32))[0].tolist()


def run_circuit(ds, fixed, own_per_copy, idx_own, shift_orders):
    """The oracle's gadgets, one copy of the verifier per entry of ds (a ProofData with hints) and of own_per_copy (the own
    values of the proof that copy verifies): all own inputs PublicInput first, then the copies.  fixed: [(idx, value)],
    idx_own: the idx of the own records.  -> the constraint system."""
    gadgets.PERMUTE = _permute
    c = C.ConstraintSystem()
    own = [[C.Var(c, tuple(v), c.new_qm31(tuple(int(x) for x in v), C.PUBLIC), 4) for v in values] for values in own_per_copy]
    for k, values in enumerate(own):
        pub = [(idx, C.qm31_constant(c, tuple(int(x) for x in val))) for idx, val in fixed] + list(zip(idx_own, values))
        verifier.verify_in_circuit(c, ds[k], pub, tuple(tuple(o) for o in shift_orders[k]))
    return c


def build_circuit(proof, inputs, n_fixed, copies=1, shift_orders=None):
    """The circuit that verifies `proof` `copies` times, inputs[n_fixed:] allocated PublicInput once per copy.
    -> (cs, ProofData)."""
    d = rc.inputs.build_inputs(proof, ob, inputs)
    own = [val for _, val in inputs[n_fixed:]]
    orders = shift_orders or [((0, -1), (0, -1))] * copies
    return run_circuit([d] * copies, inputs[:n_fixed], [own] * copies, [idx for idx, _ in inputs[n_fixed:]], orders), d


def group_circuit(proofs, inputs_per_member, n_fixed):
    """The circuit of a GROUP: copy c verifies proofs[c] under inputs_per_member[c] (the same n_fixed shared records in each),
    as tests/aggregate_ref.py builds it, with every member's own inputs PublicInput.  -> cs."""
    ds = [rc.inputs.build_inputs(p, ob, i) for p, i in zip(proofs, inputs_per_member)]
    first = inputs_per_member[0]
    return run_circuit(ds, first[:n_fixed], [[val for _, val in i[n_fixed:]] for i in inputs_per_member], [idx for idx, _ in first[n_fixed:]],
                       [((0, -1), (0, -1))] * len(proofs))


def extract(c, d, copies, n_own):
    """rc.program.extract for a circuit with own inputs: the oracle's extraction knows no public input, so it runs over a
    copy in which they pass for constants (depth 0, as an input is: the order of the instructions is the same), and their
    instructions are then written as W_INPUT."""
    import copy
    shim = copy.copy(c)
    shim.origin = list(c.origin)
    first, end = 4, 4 + copies * n_own
    for v in range(first, end):
        assert c.origin[v] == ("hint", None), (v, c.origin[v])
        shim.origin[v] = ("const",)
    prog = rc.program.extract(shim, d, copies)
    for row in prog.instr:
        if first <= row[1] < end:
            assert row[0] == rc.program.CONST
            row[:] = (W_INPUT, row[1], 0, 0, (row[1] - first) % n_own, 0, 0, 0)
    return prog


def interpret(prog, sources, own_of_variable):
    """rc.program.interpret with W_INPUT: dst = the record's value, own_of_variable(dst, imm0) -> 4 ints."""
    instr = prog.instr.copy()
    for row in instr:
        if row[0] == W_INPUT:
            row[:] = (rc.program.CONST, row[1], 0, 0) + tuple(int(x) for x in own_of_variable(int(row[1]), int(row[4])))
    return rc.program.interpret(rc.program.Program(instr, prog.level_offsets, prog.n_vars, prog.shape, prog.flow_wires), sources)


def gate_rows(c):
    return np.stack([np.array(x, dtype=np.int64) % P for x in (c.a_wire, c.b_wire, c.c_wire, c.op, c.poseidon_wire, c.enforce_c_m31)], axis=1)


def write_hints(path, proof, inputs, copies, walks):
    """The hints file tests/host_logic_asan.cpp documents, from the C oracle (the records in the order of `inputs`)."""
    d = rc.parse_proof(proof)
    sib, pos, _ = ob.trace_paths(proof, d.nq, d.M, inputs)
    fsib, fcols = ob.fri_paths(proof, d.nq, d.M, 1 + d.n_inner, inputs)
    tcols = ob.trace_cols(proof, inputs)
    flow = ob.poseidon_flow(proof, inputs)
    count = flow.shape[0]

    def padded(b):
        b = np.frombuffer(bytes(b), dtype=np.uint8)
        return np.concatenate([b, np.zeros((-len(b)) % 4, np.uint8)]).view(np.uint32)

    pi = np.array([[idx] + [int(x) for x in val] for idx, val in inputs], dtype=np.uint32).reshape(-1)
    hdr = np.zeros(16, np.uint32)
    hdr[:8] = [0x52535648, len(proof), d.nq, d.M, d.n_inner, count, len(inputs), copies]
    parts = [hdr, padded(proof), sib.reshape(-1), pos.reshape(-1), tcols.reshape(-1), fsib.reshape(-1), fcols.reshape(-1),
             np.ascontiguousarray(flow[:, :32]).reshape(-1), padded(flow[:, 32].astype(np.uint8)), pi, padded(bytes(walks))]
    np.concatenate([np.ascontiguousarray(p, dtype=np.uint32) for p in parts]).tofile(path)


def read_program(path):
    """The file tests/witness_inputs_host.cpp writes -> dict of arrays."""
    w = np.fromfile(path, dtype=np.uint32)
    assert w[0] == 0x52535651
    n_vars, n_levels, n_fw, n_gates, n_wo, num_input = (int(x) for x in w[1:7])
    at = 8
    out = {"n_vars": n_vars, "num_input": num_input}
    for name, count, shape in (("instr", 8 * n_vars, (n_vars, 8)), ("levels", n_levels + 1, (-1,)), ("flow_wires", n_fw, (-1, 5)),
                               ("gates", n_gates, (-1, 6)), ("witness_ops", n_wo, (-1, 3)), ("copy_of", n_vars, (-1,))):
        out[name] = w[at:at + count].reshape(shape)
        at += count
    assert at == len(w)
    return out
