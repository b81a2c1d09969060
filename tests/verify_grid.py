"""What the tests of the configuration grid share (no test lives here): a table of PCS configurations that no fixture has,
on five circuit shapes the chain can prove, and generate(), which makes one genuine proof at a point of it.  The verifier
promises every configuration rsv_cfg_check admits; the fixtures and the chain's other tests reach ten of them.  The grid
puts a genuine proof on both sides of every place where the verifier's code changes with the configuration:

  n_queries   G = max(n_queries, 4) (dead lanes below four), 32 / 33 (the last geometry of the row forms and the first
              that falls back to the lane forms), 64 / 65 and 128 (one proof's queries span two waves; the plan's 8-bit
              fields at their largest), on a domain of 2^7 positions where 128 queries collide and on one of 2^17 where
              they stay distinct;
  log_last    0, 1, 3, 4, 5 (on either side of line_eval's block loop), 6 and 9 .. 14 (a thread of the row form holds more
              than one block of 16 coefficients); a shape takes log_last up to min(lp, lq) - 2 (provable(): one more and its
              smallest column would meet no inner layer, rsv_witness_fri_dev refuses);
  log_blowup  4, 6, 10 and 16, the limit (S1: M = 26; generating that proof takes 0.18 s on an MI355X);
  pow_bits    0 and 24.

Shapes: S1, S2, S3 of tests/user_circuit_ref.py, (lp, lq) = (6, 8), (12, 8), (7, 9); R, the recursion circuit of the
level10-1 -> level11-1 pair, (16, 15); and R17, that of the level2-1 -> level3-1 pair, (17, 16), the smallest shape that
takes log_last = 14.  Nothing generated is stored: tests/test_verify_grid_gpu.py makes every proof once
per run; tests/test_verify_grid_host.py checks the table without a device."""
import numpy as np

from tests import user_circuit_ref as U
from tests.chain_harness import DEV, FILL, header_logs, inputs_of, pin_of, program_of, tail, whole_chain
from tests.conftest import read_proof

R_SRCS = {"R": "level10-1.bin", "R17": "level2-1.bin"}     # the fixture whose recursion circuit the shape is
SHAPES = ("S1", "S2", "S3", "R", "R17")

# (shape, pow_bits, log_blowup, log_last, n_queries)
Q_SMALL = (1, 2, 3, 4, 5, 15, 17, 31, 32, 33, 63, 64, 65, 127, 128)
Q_LARGE = (1, 4, 32, 33, 64, 65, 128)
POINTS = (
    # Q axis, small domain: the Plonk columns' domain has 2^7 positions, 128 queries saturate it (and the largest column's
    # 2^11 leave few nonces whose queries are distinct there: generate() takes the first)
    [("S1", 2, 1, 0, nq) for nq in Q_SMALL]
    # Q axis, large domain: M = 18, the queries stay distinct
    + [("R", 2, 1, 8, nq) for nq in Q_LARGE]
    # L axis
    + [("S2", 2, 2, ll, 6) for ll in (1, 3, 4, 5, 6)]       # 6: the largest S2 allows
    + [("R", 2, 1, ll, 16) for ll in (9, 10, 12, 13)]      # 13: the largest R allows, n_inner = 3
    + [("R17", 2, 1, 14, 16)]                               # n_inner = 3
    + [("S1", 2, 1, 4, 12)]                                 # the largest S1 allows, n_inner = 5
    # B axis
    + [("S3", 2, b, 2, 7) for b in (4, 6, 10)]
    + [("S1", 2, 16, 2, 7)]                                 # RSV_MAX_LOG_BLOWUP: M = 26
    # P axis
    + [("S1", 0, 1, 0, 9), ("S1", 24, 1, 0, 9)]
)


def point_id(point):
    return "%s-pow%d-blowup%d-last%d-q%d" % point


def logs_of(shape):
    """(lp, lq) of a shape, computed on the CPU: the oracle's columns of an S circuit, the header of R's next fixture."""
    if shape in R_SRCS:
        return header_logs(pin_of(R_SRCS[shape])["dst"])
    return U.columns(U.build(shape))[4:6]


def sizes_of(lp, lq, point):
    """The oracle's rule (oracle/rsv_oracle.c) -> (M, A, B, n_inner): the largest quotient column's LDE log size, the Plonk
    and the Poseidon columns', and the inner FRI layers."""
    _shape, _pow, b, ll, _nq = point
    M = max(lp + 1, lq + 2) + b
    return M, lp + b, lq + b, M - 1 - ll - b


def provable(lp, lq, point):
    """Whether an accepting proof exists at the point: every column's circle-to-line fold must land on an inner layer, above
    the last layer's 2^(log_last + log_blowup) values.  The reference's prover asserts it and its verifier folds nothing in
    behind the last inner layer (components/recursive/folding/src/lib.rs); rsv_witness_fri_dev refuses the rest."""
    return min(lp, lq) >= point[3] + 2


# ---------------------------------------------------------------- the chain of a caller's circuit
def _finish(ch, cfg, distinct=False):
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch, stage)()
    return tail(ch, cfg, distinct)


def _run(rsv, ctx, circ, builts, config, check=True, flows=None, distinct=False):
    cfg = rsv.PcsConfig(*config)
    ch = rsv.Chain(ctx, circ, len(builts), cfg.log_blowup_factor, log_last=cfg.log_last_layer_degree_bound, fill=FILL, caps=True, device=DEV)
    flows = [b.unbound_flow() if check else b.flow for b in builts] if flows is None else flows
    ch.load(np.stack([b.variables for b in builts]), np.stack(flows), None if check else np.stack([b.swap for b in builts]), check=check)
    return _finish(ch, cfg, distinct), cfg


# ---------------------------------------------------------------- one genuine proof at a point
class Programs:
    """The programs of the five shapes, built on first use and closed together."""

    def __init__(self, rsv):
        self.rsv, self.built, self.prog = rsv, {}, {}

    def of(self, shape):
        if shape not in self.prog:
            if shape in R_SRCS:
                self.prog[shape] = program_of(self.rsv, pin_of(R_SRCS[shape]))
            else:
                b = self.built[shape] = U.build(shape)
                self.prog[shape] = self.rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, b.witness_ops)
        return self.prog[shape]

    def close(self):
        for p in self.prog.values():
            p.close()
        self.prog = {}


def generate(rsv, ctx, point, programs=None):
    """-> (proof bytes, cfg, the public inputs it verifies under) of one genuine proof at `point`.  programs: a Programs
    to share over many points (the caller closes it)."""
    shape, config = point[0], point[1:]
    own = programs is None
    programs = Programs(rsv) if own else programs
    try:
        prog = programs.of(shape)
        cfg = rsv.PcsConfig(*config)
        if shape in R_SRCS:
            src = R_SRCS[shape]
            got, proofs = whole_chain(rsv, ctx, prog, [read_proof(src)], inputs_of(src), cfg, distinct=True)
            assert got["ok"].tolist() == [1] and proofs[0] is not None, point
            return proofs[0], cfg, inputs_of(pin_of(src)["dst"])
        b = programs.built[shape]
        ch, cfg = _run(rsv, ctx, prog, [b], config, distinct=True)
        blob, offsets = ch.pack(exact=True)                    # the device's serialiser: no tensor but the proof comes back
        assert offsets.cpu().tolist()[1] > 0 and ch.ok.cpu().tolist() == [1], point
        return blob.cpu().numpy().tobytes(), cfg, b.inputs
    finally:
        if own:
            programs.close()
