"""What the tests of the statement digest share (no test lives here): the sponge of hash_m31_columns_get_rate restated over
the C oracle's permutation, state by state, and the same hash run through the oracle's circuit gadgets
(oracle/recursion_circuit, used as it is).

The definition (include/rsv.h, rsv_statement_digest_dev): a group of `copies` proofs with n_own records each has the words
v[c * n_own + k] = value[0] of record k of proof c, T = copies * n_own of them, and its digest is
hash_m31_columns_get_rate(v) = tests/oracle_binding.hash_node(None, v); the statement made of it is eight records
(4 + k, (digest[k], 0, 0, 0))."""
import numpy as np

from oracle.recursion_circuit import cs as C
from oracle.recursion_circuit import gadgets
from tests import oracle_binding as ob

P = C.P
T_CASES = (1, 7, 8, 9, 16, 17, 67, 134)   # one chunk, a full chunk, two full chunks (remain == 0), remainders; 134 = two copies of 67


def sponge_states(v):
    """The S = ceil(T / 8) + 1 invocations of the hash of the words v, in order: [(left[8], right[8], out[16])], swap 0 in
    all of them.  The digest is the first half of the last `out`."""
    v = [int(x) for x in v]
    assert v and all(0 <= x < P for x in v)
    states, d = [], [0] * 8
    for off in range(0, len(v), 8):
        chunk = (v[off:off + 8] + [0] * 8)[:8]
        out = ob.poseidon2_permute(np.array(chunk + d, dtype=np.uint32))[0].tolist()
        states.append((chunk, d, out))
        d = out[8:]
    out = ob.poseidon2_permute(np.array([0] * 8 + d, dtype=np.uint32))[0].tolist()
    states.append(([0] * 8, d, out))
    return states


def digest(v):
    return sponge_states(v)[-1][2][:8]


def statement_records(rec, copies):
    """rec uint32[n_groups * copies, n_own, 5] -> (stmt uint32[n_groups, 8, 5], bad uint8[n_groups]) by the rules of the
    kernel: a value word >= P counts as 0 and sets bad, a non-zero word 1..3 of the value sets bad."""
    rec = np.asarray(rec, dtype=np.uint32)
    n_own = rec.shape[1]
    groups = rec.reshape(-1, copies * n_own, 5)
    stmt = np.zeros((groups.shape[0], 8, 5), np.uint32)
    bad = np.zeros(groups.shape[0], np.uint8)
    for g, r in enumerate(groups):
        v = r[:, 1].astype(np.int64)
        bad[g] = 1 if (v >= P).any() or r[:, 2:].any() else 0
        v[v >= P] = 0
        stmt[g, :, 0] = 4 + np.arange(8)
        stmt[g, :, 1] = digest(v)
    return stmt, bad


def gadget_digest(v):
    """The same hash by the oracle's circuit gadget over M31 witness variables: -> (digest[8], the constraint system)."""
    gadgets.PERMUTE = lambda state: ob.poseidon2_permute(np.array(state, dtype=np.uint32))[0].tolist()
    c = C.ConstraintSystem()
    own = [C.m31_witness(c, int(x)) for x in v]
    h = gadgets.hash_m31_columns_get_rate(own)
    return [int(x) for x in h.value], c


# ---------------------------------------------------------------- the hashed program (rsv_witness_program_build_inputs_hashed)
# The outer circuit, in allocation order: the statement, eight PublicInput M31 variables 4 .. 11 (W_STMT, imm0 = word); the own
# records, M31 WITNESS variables 12 .. 12 + T copy-major (W_INPUT, imm0 = k); half_equalverify(half_from_m31(statement),
# hash_m31_columns_get_rate(own)); the copies of the verifier.  The hash's S invocations take the flow indices behind the
# copies' (copies * F ..), whatever the order the gadgets ran in.
W_INPUT, W_STMT = 19, 20        # layout.hpp: behind W_FRI_COL (18)


def flow_records(v):
    """The hash's records as the kernel writes them: uint32[S, 32] = left | right | out."""
    return np.array([l + r + o for l, r, o in sponge_states(v)], dtype=np.uint32)


def run_circuit(ds, fixed, own_per_copy, idx_own, shift_orders):
    """The oracle's gadgets with the layout above, one copy of the verifier per entry of ds (ProofData with hints) and of
    own_per_copy (the own values of the proof that copy verifies).  -> the constraint system."""
    from oracle.recursion_circuit import verifier
    gadgets.PERMUTE = lambda state: ob.poseidon2_permute(np.array(state, dtype=np.uint32))[0].tolist()
    c = C.ConstraintSystem()
    words = [int(v[0]) for values in own_per_copy for v in values]
    assert all(tuple(int(x) for x in v[1:]) == (0, 0, 0) for values in own_per_copy for v in values)
    stated = [C.Var(c, w, c.new_m31(w, C.PUBLIC), 1) for w in digest(words)]
    own = [[C.m31_witness(c, int(v[0])) for v in values] for values in own_per_copy]
    gadgets.half_equalverify(gadgets.half_from_m31(stated), gadgets.hash_m31_columns_get_rate([x for values in own for x in values]))
    for k, values in enumerate(own):
        pub = [(idx, C.qm31_constant(c, tuple(int(x) for x in val))) for idx, val in fixed] + list(zip(idx_own, values))
        verifier.verify_in_circuit(c, ds[k], pub, tuple(tuple(o) for o in shift_orders[k]))
    return c


def build_circuit(proof, inputs, n_fixed, copies=1, shift_orders=None):
    """The hashed circuit that verifies `proof` `copies` times under inputs[n_fixed:] as own records.  -> (cs, ProofData)."""
    from oracle import recursion_circuit as rc
    d = rc.inputs.build_inputs(proof, ob, inputs)
    own = [val for _, val in inputs[n_fixed:]]
    orders = shift_orders or [((0, -1), (0, -1))] * copies
    return run_circuit([d] * copies, inputs[:n_fixed], [own] * copies, [idx for idx, _ in inputs[n_fixed:]], orders), d


def group_circuit(proofs, inputs_per_member, n_fixed):
    """The hashed circuit of a GROUP: copy c verifies proofs[c] under inputs_per_member[c].  -> cs."""
    from oracle import recursion_circuit as rc
    ds = [rc.inputs.build_inputs(p, ob, i) for p, i in zip(proofs, inputs_per_member)]
    first = inputs_per_member[0]
    return run_circuit(ds, first[:n_fixed], [[val for _, val in i[n_fixed:]] for i in inputs_per_member], [idx for idx, _ in first[n_fixed:]],
                       [((0, -1), (0, -1))] * len(proofs))


def extract(c, d, copies, n_own):
    """rc.program.extract for a hashed circuit.  The oracle's extraction knows neither a public input nor a flow index
    behind the copies', so it runs over a copy of the system in which the statement, the own records and the outputs of the
    hash pass for constants (depth 0, as they are) and the flow is in the program's order — the copies' records, then the
    hash's — and their instructions are then written as W_STMT, W_INPUT and W_FLOW with the tail's index."""
    import copy
    from oracle import recursion_circuit as rc
    T = copies * n_own
    S = -(-T // 8) + 1
    F = (len(c.flow) - S) // copies
    assert len(c.flow) == copies * F + S
    shim = copy.copy(c)
    shim.origin = list(c.origin)
    shim.flow = list(c.flow[S:]) + list(c.flow[:S])
    patched = {}
    for v, origin in enumerate(c.origin):
        if 4 <= v < 12 + T:
            assert origin == ("hint", None), (v, origin)
            patched[v] = (W_STMT, v, 0, 0, v - 4, 0, 0, 0) if v < 12 else (W_INPUT, v, 0, 0, (v - 12) % n_own, 0, 0, 0)
        elif origin[0] == "hint" and origin[1] is not None and origin[1][0] == "perm":
            tag = origin[1]
            if tag[1] < S:
                patched[v] = (rc.program.FLOW, v, 0, 0, copies * F + tag[1], 16 + 8 * tag[2] + 4 * tag[3], 0, 0)
            else:
                shim.origin[v] = ("hint", ("perm", (tag[1] - S) % F) + tuple(tag[2:]))
        if v in patched:
            shim.origin[v] = ("const",)
    assert sum(1 for r in patched.values() if r[0] == rc.program.FLOW) == 2 * S
    prog = rc.program.extract(shim, d, copies)
    for row in prog.instr:
        if int(row[1]) in patched:
            assert row[0] == rc.program.CONST
            row[:] = patched[int(row[1])]
    return prog, F, S


def interpret(prog, sources, own_of_variable, statement):
    """rc.program.interpret with W_INPUT (own_of_variable(dst, imm0) -> 4 ints) and W_STMT (statement[imm0])."""
    from oracle import recursion_circuit as rc
    instr = prog.instr.copy()
    for row in instr:
        if row[0] == W_INPUT:
            row[:] = (rc.program.CONST, row[1], 0, 0) + tuple(int(x) for x in own_of_variable(int(row[1]), int(row[4])))
        elif row[0] == W_STMT:
            row[:] = (rc.program.CONST, row[1], 0, 0, int(statement[int(row[4])]), 0, 0, 0)
    return rc.program.interpret(rc.program.Program(instr, prog.level_offsets, prog.n_vars, prog.shape, prog.flow_wires), sources)
