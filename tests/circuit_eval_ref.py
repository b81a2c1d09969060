"""What the tests of rsv_circuit_program_create_eval / rsv_circuit_eval_dev share (no test lives here): the hints, links and
input buffer of a circuit built with the oracle's constraint system (oracle/recursion_circuit/cs.py keeps an `origin` for
every variable), a Python-integer interpreter of an EXPORTED evaluation program, and a fourth circuit beside
tests/user_circuit_ref.py's S1 to S3.

  S4  every hint kind: m31_inv of a non-zero value, m31_is_zero of a zero and of a non-zero value, qm31_inv, cm31_inv (both
      coordinates), decompose_m31 (all four), a copy, a 5-bit decomposition; a new_qm31(CONSTANT), whose defining row comes
      after rows that use higher-numbered variables; a witness-op row; 8 independent invocations on one level; a sponge
      chain of 22 dependent permutations linked through ignored outputs; swap bits that are computed variables (an
      is_zero output equal to 1, and one equal to 0).

The hints carry only what the gate list cannot say: ("hint", ("perm", ...)) origins are left for rule 3 to find, const / add
/ mul / mulc for rule 4 (include/rsv.h has the rule)."""
import numpy as np

from oracle.recursion_circuit import cs as C
from oracle.recursion_circuit import gadgets as G
from tests import oracle_binding as ob
from tests import user_circuit_ref as U
from tests.chain_harness import P

KINDS = U.KINDS + ("S4",)
INPUT, COPY, INV, INV0, QINV, CINV, COORD, BIT = range(8)
_KIND_OF = {"copy": COPY, "inv": INV, "inv_or_zero": INV0, "qinv": QINV, "cinv": CINV, "coord": COORD, "bit": BIT}
E_INPUT, E_GATE = 32, 33


# ---------------------------------------------------------------- the arrays of a built circuit
def hints_of(cs):
    """-> uint32[n_hints, 4] = (dst, kind, src, imm) from cs.origin; the INPUT slots count up in variable order."""
    out, slot = [], 0
    for v, o in enumerate(cs.origin):
        if o[0] != "hint":
            continue                                   # const, add, mul, mulc: rule 4
        tag = o[1]
        if tag is None:
            out.append((v, INPUT, 0, slot))
            slot += 1
        elif tag[0] == "perm":
            continue                                   # rule 3
        else:
            out.append((v, _KIND_OF[tag[0]], tag[1], tag[2] if len(tag) > 2 else 0))
    return np.array(out, dtype=np.uint32).reshape(-1, 4)


class _Links:
    """gadgets.permute wrapped while a circuit is built: an input Half without a wire that IS (the same object as) an
    ignored output of an earlier permutation is linked to it.  The rows end up in cs.links."""

    def __enter__(self):
        self.inner, self.out, self.keep = G.permute, {}, []
        G.permute = self
        return self

    def __exit__(self, *exc):
        G.permute = self.inner

    def __call__(self, left, right, ignore_left, ignore_right, is_swap=None):
        cs = left.cs
        k = len(cs.flow)
        row = [self.out.get(id(h), 0) if h.sel == 0 else 0 for h in (left, right)]
        new = self.inner(left, right, ignore_left, ignore_right, is_swap=is_swap)
        self.keep += [left, right, *new]               # ids stay unique while the objects live
        for h, half in enumerate(new):
            if half.sel == 0:
                self.out[id(half)] = 1 + 2 * k + h
        cs.__dict__.setdefault("links", []).append(row)
        return new


def links_of(cs):
    """-> uint32[n_flow, 2]: 0, or 1 + 2 k' + h' (see _Links)."""
    links = np.array(getattr(cs, "links", []), dtype=np.uint32).reshape(-1, 2)
    assert len(links) == len(cs.flow)
    return links


def inputs_of(built):
    """-> uint32[n_inputs, 4]: the values of the INPUT hints' variables, by slot."""
    h = hints_of(built.cs)
    h = h[h[:, 1] == INPUT]
    out = np.zeros((len(h), 4), np.uint32)
    out[h[:, 3]] = built.variables[h[:, 0]]
    return out


def flow_in_of(built):
    """The flow as rsv_circuit_eval_dev takes it: only the input halves with neither a wire nor a link."""
    links = links_of(built.cs)
    f = np.zeros_like(built.flow)
    for h in range(2):
        free = (built.flow_wires[:, h] == 0) & (links[:, h] == 0)
        f[free, 8 * h:8 * h + 8] = built.flow[free, 8 * h:8 * h + 8]
    return f


def _s4(pub, seed, bit):
    G.PERMUTE = U.permute
    c = C.ConstraintSystem()
    rnd = np.random.default_rng(seed)
    q = lambda: tuple(int(x) for x in rnd.integers(0, P, 4))
    oct_ = lambda: [int(v) for v in rnd.integers(0, P, 8)]
    x = C.Var(c, tuple(pub), c.new_qm31(tuple(pub), C.PUBLIC), 4)
    a = C.qm31_witness(c, q())
    w = C.m31_witness(c, int(rnd.integers(1, P)))
    w2 = C.m31_witness(c, int(rnd.integers(1, P)))
    wi = C.m31_inv(w)                                              # INV
    is1 = C.m31_is_zero(C.sub(w, w))                               # INV0 of 0: the output is 1
    is0 = C.m31_is_zero(w)                                         # INV0 of a non-zero value: the output is 0
    assert (is1.value, is0.value) == (1, 0)
    qi = C.qm31_inv(a)                                             # QINV
    ci = C.cm31_inv(C.cm31_from_m31(w, w2))                        # CINV 0 and 1
    parts = C.decompose_m31(a)                                     # COORD 0..3
    cp = C.qm31_witness(c, a.value, ("copy", a.variable))          # COPY
    small = C.m31_witness(c, int(rnd.integers(0, 32)))
    bits = G.bits_from_m31(small, 5)                               # BIT 0..4
    y = C.mul(C.add(x, qi), C.add(cp, wi))
    y = C.add(y, C.mul(ci, parts[3]))
    y = C.add(y, C.Var(c, 1 if bits.value[2] else 0, bits.variables[2], 1))
    y = C.mul(y, C.qm31_constant(c, (5, 6, 7, 8)))                 # new_qm31(CONSTANT): its row follows its parts' rows
    b = C.m31_witness(c, bit)
    witness_ops = [(c.num_plonk_rows(), b.variable, U.OP_CONSTANT)]
    sel = C.Var(c, U.OP_CONSTANT * bit % P, c.mul_constant(b.variable, U.OP_CONSTANT if bit else 0), 1)
    y = C.add(y, sel)
    # 8 independent invocations: every input half is a pair of inputs
    wide = [G.permute(G.half_witness(c, oct_()), G.half_witness(c, oct_()), False, k % 2 == 0) for k in range(8)]
    for left, _ in wide:
        y = C.add(y, left.to_qm31()[1])
    # the sponge: 22 permutations, each fed by the ignored outputs of the one before, two of them under a computed swap bit
    l, r = G.permute(G.half_from_qm31(y, a), G.half_single_use(c, oct_()), True, True)
    for k in range(20):
        swap = (1, is1.variable) if k == 3 else (0, is0.variable) if k == 4 else None
        l, r = G.permute(l, r, True, True, is_swap=swap)
    l, r = G.permute(l, r, False, False)
    y = C.mul(C.add(l.to_qm31()[0], r.to_qm31()[1]), y)            # bound outputs read by later gates
    G.permute(G.half_from_qm31(y, x), wide[1][1], False, True)
    return U.Built(c, witness_ops)


def build(kind, pub=(11, 0, 0, 0), seed=1, bit=1):
    """S1 to S3 of tests/user_circuit_ref.py and S4, built under the link recorder: Built, with cs.links."""
    assert kind in KINDS
    with _Links():
        b = _s4(pub, seed, bit) if kind == "S4" else U.build(kind, pub=pub, seed=seed, bit=bit)
    b.cs.check_arithmetics()
    b.cs.check_poseidon_invocations(U.permute)
    return b


def create_args(b):
    """The keyword arguments of rsv.Circuit for the evaluation program of a Built."""
    return dict(witness_ops=b.witness_ops, hints=hints_of(b.cs), flow_links=links_of(b.cs), n_inputs=len(inputs_of(b)))


# ---------------------------------------------------------------- the interpreter
def flow_sources(gates, flow_wires):
    """-> int64[n_flow, 4, 2]: (a_wire, b_wire) of the row that carries the wire of r1..r4, (-1, -1) without a wire."""
    g = np.asarray(gates, np.int64)
    row_of = {int(r[4]): i for i, r in enumerate(g) if r[4]}
    out = np.full((len(flow_wires), 4, 2), -1, np.int64)
    for k, fw in enumerate(np.asarray(flow_wires, np.int64)):
        for h in range(4):
            if fw[h]:
                out[k, h] = g[row_of[int(fw[h])], :2]
    return out


def model_eval(instr, levels, flow_order, flow_levels, tables, inputs, flow_in):
    """An exported program run on Python integers, level by level: a level's instructions, then its invocations.
    tables = (gates, flow_wires, flow_links, n_vars).  -> (variables uint32[n_vars, 4], flow uint32[n_flow, 32], swap
    uint8[n_flow]).  A variable read before it is written is an AssertionError; the output variables of an invocation are
    the wires of its r3 / r4 rows that no instruction defines."""
    gates, flow_wires, links, n_vars = tables
    src = flow_sources(gates, flow_wires)
    fw = np.asarray(flow_wires, np.int64)
    instr = np.asarray(instr, np.int64)
    by_instr = set(int(d) for d in instr[:, 1])
    v = [None] * n_vars
    flow = [[int(x) for x in row] for row in np.asarray(flow_in, np.int64).reshape(len(fw), 32)]
    done = [False] * len(fw)
    swap = [0] * len(fw)

    def rd(k):
        assert v[k] is not None, ("read before written", k)
        return v[k]

    def put(k, val):
        assert v[k] is None, ("defined twice", k)
        v[k] = tuple(int(x) for x in val)

    for l in range(len(levels) - 1):
        for op, dst, a, b, i0, i1, i2, _ in instr[levels[l]:levels[l + 1]].tolist():
            if op == 0:
                r = (i0, i1, i2, _)
            elif op == 1:
                r = C.q_add(rd(a), rd(b))
            elif op == 2:
                r = C.q_mul(rd(a), rd(b))
            elif op == 3:
                r = C.q_scale(rd(a), i0)
            elif op == 4:
                r = rd(a)
            elif op in (5, 6):
                r = (C.m_inv(rd(a)[0]), 0, 0, 0)
            elif op == 7:
                r = C.q_inv(rd(a)) if any(rd(a)) else C.ZERO4
            elif op == 8:
                r = (C.c_inv(rd(a)[:2])[i0] if any(rd(a)[:2]) else 0, 0, 0, 0)
            elif op == 9:
                r = (rd(a)[i0], 0, 0, 0)
            elif op == 10:
                r = ((rd(a)[0] >> i0) & 1, 0, 0, 0)
            elif op == E_INPUT:
                r = tuple(int(x) for x in inputs[i0])
            elif op == E_GATE:
                k = (i0 if rd(i1)[0] else 0) if i2 else i0
                r = C.q_add(C.q_scale(C.q_add(rd(a), rd(b)), k), C.q_scale(C.q_mul(rd(a), rd(b)), (1 - k) % P))
            else:
                raise AssertionError(("unknown op", op))
            put(dst, r)
        for k in [int(x) for x in flow_order[flow_levels[l]:flow_levels[l + 1]]]:
            for h in range(2):
                if fw[k, h]:
                    flow[k][8 * h:8 * h + 8] = list(rd(src[k, h, 0])) + list(rd(src[k, h, 1]))
                elif links[k][h]:
                    kk, hh = divmod(int(links[k][h]) - 1, 2)
                    assert done[kk], ("linked before it ran", k, kk)
                    flow[k][8 * h:8 * h + 8] = flow[kk][16 + 8 * hh:24 + 8 * hh]
            swap[k] = rd(fw[k, 4])[0] & 1 if fw[k, 4] else 0
            state = flow[k][8:16] + flow[k][:8] if swap[k] else flow[k][:16]
            flow[k][16:] = U.permute(state)
            done[k] = True
            for h in (2, 3):
                for s in range(2):
                    var = int(src[k, h, s])
                    if var >= 4 and var not in by_instr:
                        put(var, flow[k][8 * h + 4 * s:8 * h + 4 * s + 4])
    assert all(done) and all(x is not None for x in v), [k for k, x in enumerate(v) if x is None][:8]
    return np.array(v, dtype=np.uint32), np.array(flow, dtype=np.uint32), np.array(swap, dtype=np.uint8)
