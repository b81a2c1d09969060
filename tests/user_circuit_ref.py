"""What the tests of a caller's own circuit share (no test lives here): three small circuits built with the oracle's
constraint system and gadgets (oracle/recursion_circuit/cs.py, gadgets.py), the arrays the library takes of them, their
expected columns (oracle/recursion_circuit/trace.py), and a numpy model of rsv_circuit_check_dev / rsv_circuit_flow_dev:
the reference's check_arithmetics and check_poseidon_invocations with the index of the first failure.

  S1  one QM31 public input (num_input = 4); an add, a mul, a mul_constant, an M31 witness (enforce_c_m31), constants, a
      row whose op follows a witness bit; six Poseidon invocations: one whose ignored output is the next one's wire-0
      input, one swapped by a witness bit equal to 1, one whose bound output a later gate reads.  < 128 rows: lp <= 7,
      lq = 8, clb = lq + 3.
  S2  S1, then a chain of multiply gates past 2^11 rows: lp = 12, lq = 8, clb = lp + 2.
  S3  S1 with 33 invocations: the padded flow is 48, lq = 9."""
import numpy as np

from oracle.recursion_circuit import cs as C
from oracle.recursion_circuit import gadgets as G
from oracle.recursion_circuit import trace as T
from tests import oracle_binding as ob
from tests.chain_harness import P, round_constants

NONE = 0xFFFFFFFF
KINDS = ("S1", "S2", "S3")
OP_CONSTANT = 987654321  # the op of S1's witness-op row where its bit is 1


def permute(state):
    return ob.poseidon2_permute(np.array(state, dtype=np.uint32))[0].tolist()


class Built:
    """A circuit and one witness of it: cs (the oracle's constraint system, before pad()), gates uint32[n_rows, 6],
    flow_wires uint32[n_flow, 5], witness_ops uint32[n, 3], n_vars, num_input, variables uint32[n_vars, 4], flow
    uint32[n_flow, 32], swap uint8[n_flow], inputs: the public inputs as (index, value) pairs."""

    def __init__(self, cs, witness_ops):
        self.cs = cs
        g = np.stack([np.array(x, dtype=np.int64) for x in (cs.a_wire, cs.b_wire, cs.c_wire, cs.op, cs.poseidon_wire, cs.enforce_c_m31)], axis=1)
        self.gates = np.ascontiguousarray(g % P, dtype=np.uint32)
        self.flow_wires = np.array([[e1[0], e2[0], e3[0], e4[0], addr] for (e1, e2, e3, e4, addr, _sw) in cs.flow], dtype=np.uint32)
        self.witness_ops = np.array(witness_ops, dtype=np.uint32).reshape(-1, 3)
        self.n_vars, self.num_input = len(cs.variables), cs.num_input
        self.variables = np.array(cs.variables, dtype=np.uint32)
        self.flow = np.array([list(e1[1]) + list(e2[1]) + list(e3[1]) + list(e4[1]) for (e1, e2, e3, e4, _a, _s) in cs.flow], dtype=np.uint32)
        self.swap = np.array([int(sw) for (*_e, sw) in cs.flow], dtype=np.uint8)
        self.inputs = [(k, tuple(int(x) for x in cs.variables[k])) for k in range(1, cs.num_input + 1)]

    def unbound_flow(self):
        """The flow as rsv_circuit_flow_dev takes it: only the input halves without a wire."""
        f = np.zeros_like(self.flow)
        for h in range(2):
            free = self.flow_wires[:, h] == 0
            f[free, 8 * h:8 * h + 8] = self.flow[free, 8 * h:8 * h + 8]
        return f


def build(kind, pub=(11, 0, 0, 0), seed=1, bit=1, public=True):
    """kind: "S1" | "S2" | "S3"; pub: the public input's value (new_qm31(PublicInput) sets enforce_c_m31 on its row, in
    the reference as here, so check_arithmetics passes a QM31 input only if it is an M31); seed: the witness values; bit: the witness bit of the
    witness-op row; public=False: the same gadgets with the input a plain witness (num_input = 3)."""
    assert kind in KINDS
    G.PERMUTE = permute
    c = C.ConstraintSystem()
    rnd = np.random.default_rng(seed)
    q = lambda: tuple(int(x) for x in rnd.integers(0, P, 4))
    x = C.Var(c, tuple(pub), c.new_qm31(tuple(pub), C.PUBLIC if public else C.WITNESS), 4)
    a = C.qm31_witness(c, q())
    s = C.add(x, a)
    m = C.mul(s, a)
    k = C.mul_constant(m, 12345)
    w = C.m31_witness(c, int(rnd.integers(0, P)))             # enforce_c_m31
    k = C.add(k, C.mul(w, C.m31_constant(c, 4242)))           # a constant's row
    k = C.mul(k, C.qm31_constant(c, (5, 6, 7, 8)))
    one = C.m31_witness(c, 1)                                 # the swap bit: a witness equal to 1
    b = C.m31_witness(c, bit)                                 # the bit the witness-op row follows
    witness_ops = [(c.num_plonk_rows(), b.variable, OP_CONSTANT)]
    sel = C.Var(c, OP_CONSTANT * bit % P, c.mul_constant(b.variable, OP_CONSTANT if bit else 0), 1)
    k = C.add(k, sel)
    h1 = G.half_witness(c, [int(v) for v in rnd.integers(0, P, 8)])
    h2 = G.half_from_qm31(m, k)
    l1, r1 = G.permute(h1, h2, False, True)                   # r1 is ignored ...
    _, r2 = G.permute(l1, r1, True, False)                    # ... and is this one's wire-0 input
    l3, _ = G.permute(r2, G.half_zero(c), False, True, is_swap=(1, one.variable))
    l4, r4 = G.permute(l3, G.half_zero(c), False, False)
    y = C.add(l4.to_qm31()[0], x)                             # a bound output read by a later gate
    y = C.mul(y, r4.to_qm31()[1])
    l5, r5 = G.permute(G.half_from_qm31(y, a), G.half_single_use(c, [int(v) for v in rnd.integers(0, P, 8)]), True, True)
    G.permute(l5, r5, True, True)                             # nothing of it is bound
    if kind == "S3":
        cl, cr = G.permute(h1, G.half_zero(c), False, True)
        while len(c.flow) < 33:
            cl, cr = G.permute(cl, cr, False, True)
    if kind == "S2":
        while c.num_plonk_rows() <= (1 << 11):
            y = C.mul(y, a)
    return Built(c, witness_ops)


def columns(b):
    """The oracle's columns of a built circuit: (plonk pre [10, N], plonk trace [12, N], poseidon pre [40, Q], poseidon
    trace [48, Q], lp, lq), after pad() of a copy of the constraint system."""
    import copy
    c = copy.deepcopy(b.cs)
    N = T.pad(c)
    lp = N.bit_length() - 1
    lq = (6 * len(c.flow) - 1).bit_length()
    pre, tr = T.plonk_columns(c)
    ppre = np.stack([np.asarray(pre[k], dtype=np.int64) % P for k in T.PREPROCESSED])
    qpre, qtr = T.poseidon_columns(c.flow, round_constants(), lq, padding_hash=([0] * 8,))
    return ppre, np.asarray(tr, np.int64), qpre.astype(np.int64), qtr.astype(np.int64), lp, lq


# ---------------------------------------------------------------- the model
def _qmul(a, b):
    m = lambda x, y: x * y % P
    a0, a1, a2, a3 = (a[:, k] for k in range(4))
    b0, b1, b2, b3 = (b[:, k] for k in range(4))
    ac0, ac1 = m(a0, b0) - m(a1, b1), m(a0, b1) + m(a1, b0)
    bd0, bd1 = m(a2, b2) - m(a3, b3), m(a2, b3) + m(a3, b2)
    ad0, ad1 = m(a0, b2) - m(a1, b3), m(a0, b3) + m(a1, b2)
    bc0, bc1 = m(a2, b0) - m(a3, b1), m(a2, b1) + m(a3, b0)
    return np.stack([ac0 + 2 * bd0 - bd1, ac1 + 2 * bd1 + bd0, ad0 + bc0, ad1 + bc1], axis=1) % P


def model_check(gates, witness_ops, variables):
    """check_arithmetics over `variables` uint32[n_vars, 4] -> the first failing row, or NONE.  A row fails if
    c != op (a + b) + (1 - op) a b, if enforce_c_m31 is set and c is no M31, if a word it reads is not below P, or, for
    the rows 0..3, if the variable is not 0, 1, i, j."""
    g = np.asarray(gates, np.int64)
    v = np.asarray(variables, np.int64)
    op = g[:, 3] % P
    ops = np.asarray(witness_ops, np.int64).reshape(-1, 3)
    if len(ops):
        op[ops[:, 0]] = np.where(v[ops[:, 1], 0] != 0, ops[:, 2] % P, 0)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    want = ((a + b) % P * op[:, None] + _qmul(a, b) * ((1 - op) % P)[:, None]) % P
    bad = (want != c).any(axis=1) | (a >= P).any(axis=1) | (b >= P).any(axis=1) | (c >= P).any(axis=1)
    bad |= (g[:, 5] != 0) & (c[:, 1:] != 0).any(axis=1)
    bad[:4] |= (v[:4] != np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])).any(axis=1)
    rows = np.flatnonzero(bad)
    return int(rows[0]) if len(rows) else NONE


def model_flow(gates, flow_wires, variables, flow_in):
    """check_poseidon_invocations over `variables`, making the flow -> (the first failing invocation or NONE, flow
    uint32[n_flow, 32], swap uint8[n_flow]).  An input half with a wire is (variables[a_wire], variables[b_wire]) of the
    row that carries it, one without is read from flow_in; invocation k fails if an input word is not below P, if the
    swap bit is not the QM31 0 or 1, or if an output with a wire is not its pair in `variables`."""
    g, fw, v = np.asarray(gates, np.int64), np.asarray(flow_wires, np.int64), np.asarray(variables, np.int64)
    row_of = {int(r[4]): i for i, r in enumerate(g) if r[4]}
    n = len(fw)
    flow = np.array(flow_in, dtype=np.int64).reshape(n, 32).copy()
    bound = np.zeros((n, 4, 8), np.int64)
    for k in range(n):
        for h in range(4):
            if fw[k, h]:
                r = g[row_of[int(fw[k, h])]]
                bound[k, h] = np.concatenate([v[r[0]], v[r[1]]])
                if h < 2:
                    flow[k, 8 * h:8 * h + 8] = bound[k, h]
    bit = v[fw[:, 4]]
    bad = (flow[:, :16] >= P).any(axis=1) | ((fw[:, 4] != 0) & ((bit[:, 0] > 1) | (bit[:, 1:] != 0).any(axis=1)))
    swap = np.where(fw[:, 4] != 0, bit[:, 0] & 1, 0)
    state = np.where(swap[:, None] != 0, np.concatenate([flow[:, 8:16], flow[:, :8]], axis=1), flow[:, :16])
    state[bad] = 0
    flow[:, 16:] = ob.poseidon2_permute(state.astype(np.uint32)).astype(np.int64)
    for h in (2, 3):
        bad |= (fw[:, h] != 0) & (flow[:, 8 * h:8 * h + 8] != bound[:, h]).any(axis=1)
    ks = np.flatnonzero(bad)
    return (int(ks[0]) if len(ks) else NONE), flow.astype(np.uint32), swap.astype(np.uint8)
