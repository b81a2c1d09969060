"""What the aggregation tests share (no test lives here): the oracle's circuit of a GROUP of proofs, one copy of the verifier
per member.  It is the loop of oracle.recursion_circuit.run_circuit with one ProofData per copy instead of one for all:
verifier.verify_in_circuit once per member in one cs.ConstraintSystem.  Nothing under oracle/ changes; nothing here needs a
device."""
import functools

import numpy as np

from tests import oracle_binding as ob
from tests.chain_harness import P, inputs_of, pin_of, round_constants, walks_of
from tests.conftest import read_proof

A, B = "level10-1.bin", "level11-1.bin"  # same shape, same configuration: the existing tests batch them under A's program
COPIES = 2


def orders_of(src=A, copies=COPIES):
    """The HashSet walk orders of the pinned pair of `src` (one copy), taken for every copy of the group's circuit."""
    pin = pin_of(src)
    assert pin["multiplier"] == 1
    return [tuple(tuple(x) for x in pin["shift_orders"][0])] * copies


def walks(src=A, copies=COPIES):
    """The same as rsv_witness_program_build's set_walks."""
    return walks_of(pin_of(src)) * copies


@functools.lru_cache(maxsize=None)
def proof_data(name):
    from oracle.recursion_circuit import inputs
    return inputs.build_inputs(read_proof(name), ob, inputs_of(A))


@functools.lru_cache(maxsize=None)
def circuit(names):
    """names: a tuple of fixture names, the group's members -> (cs, marks): marks[c] = len(cs.variables) when copy c
    starts (4 for copy 0: the constraint system's four fixed constants precede it), marks[-1] = the total."""
    from oracle.recursion_circuit import cs, gadgets, verifier

    def permute(state):
        return ob.poseidon2_permute(np.array(state, dtype=np.uint32))[0].tolist()

    gadgets.PERMUTE = permute
    c = cs.ConstraintSystem()
    marks = []
    for name, order in zip(names, orders_of(copies=len(names))):
        marks.append(len(c.variables))
        pub = [(idx, cs.qm31_constant(c, tuple(int(x) for x in val))) for idx, val in inputs_of(A)]
        verifier.verify_in_circuit(c, proof_data(name), pub, order)
    marks.append(len(c.variables))
    return c, marks


def variables(names):
    return np.array(circuit(tuple(names))[0].variables, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def columns(names, lp, lq):
    """(plonk trace int64[12, 2^lp], poseidon trace int64[48, 2^lq], op column int64[2^lp]) of the group's circuit, as
    chain_harness.oracle_columns computes them for a pair.  The circuit is padded on a copy."""
    import copy

    from oracle.recursion_circuit import trace as T
    c = copy.deepcopy(circuit(tuple(names))[0])
    assert T.pad(c) == 1 << lp
    pre, tr = T.plonk_columns(c)
    _, qtr = T.poseidon_columns(c.flow, round_constants(), lq, padding_hash=([0] * 8,))
    return np.asarray(tr, np.int64), qtr.astype(np.int64), np.asarray(pre["op"], dtype=np.int64) % P
