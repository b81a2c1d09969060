"""What the chain's test modules share (no test lives here): the fixture pairs and what is read off them, the oracle's
circuit and columns of a pair, the device helpers with the tests' prefill, and chain(), which runs rsv.Chain up to a stage.
Nothing here needs a device to import; torch is imported where a helper touches one."""
import contextlib
import ctypes
import json
import os

import numpy as np

from tests import oracle_binding as ob
from tests.conftest import GOLDEN, fixture_cfg, load_manifest, read_proof

P = 0x7FFFFFFF
MAN = {e["file"]: e for e in load_manifest()}
DEV = "cuda:0"
FILL = 0xFFFFFFFF  # every output is prefilled with 0xffffffff (the uint8 flags with 7): what a call leaves undefined shows
STAGES = ("witness", "trace", "commit", "tree3", "sample", "fri")

CASES = [  # random trees: (groups as (log, cols, shared), b, n, mask)
    ([(5, 3, False)], 1, 1, None),
    ([(4, 2, False), (6, 9, False)], 3, 3, None),
    ([(6, 9, False), (4, 2, False)], 2, 2, None),
    ([(5, 4, False), (5, 12, False), (3, 1, False)], 4, 2, None),
    ([(0, 1, False), (1, 2, False), (2, 3, False), (3, 17, False)], 5, 2, None),
    ([(7, 8, False)], 9, 1, None),
    ([(6, 5, True), (5, 7, False)], 2, 4, [1, 0, 1, 1]),
    ([(3, 10, False), (2, 8, True)], 6, 5, [1, 1, 0, 1, 1]),
]

# The witness evaluation's launch forms (csrc/witness_api.inc: witness_launch), as (witness_small_max, witness_small_log,
# witness_walk_log) with None = the batch size + 1: the level-per-launch form (k_witness_level<A> below 64 proofs or groups,
# k_witness_level_wide<A> from 64 on) with its tail as a strip (k_witness_strip<A>) / in one launch of 2, 8, 64 per workgroup /
# by the default rule; the whole program in one launch (k_witness_small<A>) of 1, 4, 64 per workgroup; the default rule.
# LAUNCH_FORMS_FEW: the same without the forms of 8 and 64 per workgroup.
LAUNCH_FORMS = ((1, 0, 1), (1, 0, 2), (1, 0, 4), (1, 0, 7), (1, 0, 0), (None, 1, 0), (None, 3, 0), (None, 7, 0), (0, 0, 0))
LAUNCH_FORMS_FEW = tuple(f for f in LAUNCH_FORMS if f[1] < 7 and f[2] < 4)


@contextlib.contextmanager
def launch_form(ctx, form, n):
    """Forces a launch form on the context for a batch of n proofs (or groups); the default rule is back on exit."""
    small_max, small_log, walk_log = form
    try:
        ctx.set_option("witness_small_max", n + 1 if small_max is None else small_max)
        ctx.set_option("witness_small_log", small_log)
        ctx.set_option("witness_walk_log", walk_log)
        yield
    finally:
        for name in ("witness_small_max", "witness_small_log", "witness_walk_log"):
            ctx.set_option(name, 0)


# ---------------------------------------------------------------- the fixture pairs
def pins():
    with open(os.path.join(GOLDEN, "recursion_circuit_pins.json")) as f:
        return json.load(f)["pairs"]


def pin_id(p):
    return f"{p['src']}x{p['multiplier']}"


def pin_of(src, multiplier=None):
    return next(p for p in pins() if p["src"] == src and multiplier in (None, p["multiplier"]))


def header_logs(name):
    w = np.frombuffer(read_proof(name)[:8], np.uint32)
    return int(w[0]), int(w[1])


def inputs_of(name):
    return [(i, tuple(v)) for i, v in MAN[name]["inputs"]]


def walks_of(pin):
    orders = [tuple(tuple(x) for x in o) for o in pin["shift_orders"]]
    return [(1 if o[0] == (-1, 0) else 0) | (2 if o[1] == (-1, 0) else 0) for o in orders]


def program_of(rsv, pin):
    src = pin["src"]
    return rsv.WitnessProgram.build(read_proof(src), fixture_cfg(src), inputs_of(src), copies=pin["multiplier"], set_walks=walks_of(pin))


def lookup_of(name):
    """(z, alpha) the proof's transcript draws after trees 0 and 1."""
    tr = ob.transcript_raw(read_proof(name))
    return tuple(int(x) for x in tr[4:8]), tuple(int(x) for x in tr[8:12])


def oods_of(name):
    tr = ob.transcript_raw(read_proof(name))
    return tuple(int(x) for x in tr[20:24]), tuple(int(x) for x in tr[24:28])


def next_samples(dst):
    """sampled_values[0..2] of a fixture as uint32[134, 4], and its OODS point as uint32[8]."""
    from oracle import recursion_circuit as rc
    from tests import sample_ref as S
    nxt = read_proof(dst)
    tr = ob.transcript_raw(nxt)
    return S.flatten_samples(rc.parse_proof(nxt).sampled_values), np.array(tr[20:28], dtype=np.uint32)


def pow_words(proof):
    """The proof's nonce as the transcript mixes it: 22 / 21 / 21 bits."""
    pos = 4 * ob.proof_layout(proof)["nonce_word"]
    n = int.from_bytes(proof[pos:pos + 8], "little")
    return [n & ((1 << 22) - 1), (n >> 22) & ((1 << 21) - 1), (n >> 43) & ((1 << 21) - 1), 0]


# ---------------------------------------------------------------- the oracle's circuit and columns of a pair
def round_constants():
    ob.lib.rsvo_round_constants.restype = ctypes.POINTER(ctypes.c_uint32)
    r = [ob.lib.rsvo_round_constants(k) for k in range(3)]
    return ([[int(r[0][16 * a + i]) for i in range(16)] for a in range(4)], [int(r[1][i]) for i in range(14)],
            [[int(r[2][16 * a + i]) for i in range(16)] for a in range(4)])


def oracle_circuit(pin):
    from oracle import recursion_circuit as rc
    src = pin["src"]
    orders = [tuple(tuple(x) for x in o) for o in pin["shift_orders"]]
    c, _, _ = rc.build_circuit(read_proof(src), ob, inputs_of(src), pin["multiplier"], orders)
    gates = np.stack([np.array(x, dtype=np.int64) for x in (c.a_wire, c.b_wire, c.c_wire, c.op, c.poseidon_wire, c.enforce_c_m31)], axis=1)
    gates = np.ascontiguousarray(gates % P, dtype=np.uint32)
    wires = np.array([[e1[0], e2[0], e3[0], e4[0], addr] for (e1, e2, e3, e4, addr, _sw) in c.flow], dtype=np.uint32)
    return c, gates, wires


_COLUMNS = {}


def oracle_columns(src):
    """(plonk pre [10, N], plonk trace [12, N], poseidon pre [40, Q], poseidon trace [48, Q], lp, lq, dst) of a pair."""
    if src not in _COLUMNS:
        from oracle.recursion_circuit import trace as T
        pin = pin_of(src)
        c, _, _ = oracle_circuit(pin)
        lp, lq = header_logs(pin["dst"])
        assert T.pad(c) == 1 << lp
        pre, tr = T.plonk_columns(c)
        ppre = np.stack([np.asarray(pre[k], dtype=np.int64) % P for k in T.PREPROCESSED])
        qpre, qtr = T.poseidon_columns(c.flow, round_constants(), lq, padding_hash=([0] * 8,))
        _COLUMNS[src] = (ppre, np.asarray(tr, np.int64), qpre.astype(np.int64), qtr.astype(np.int64), lp, lq, pin["dst"])
    return _COLUMNS[src]


def weights(log_size, point):
    from oracle.recursion_circuit import trace as T
    return [np.array(w, dtype=np.int64) for w in T.PointEvaluator(log_size, point).weights]


def eval_column(w, column):
    col = np.asarray(column, dtype=np.int64)
    return tuple(int(((x * col) % P).sum() % P) for x in w)


# ---------------------------------------------------------------- the device
def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64) % (1 << 32), dtype=np.uint32).view(np.int32)).to(torch.device(DEV))


def full(shape):
    import torch
    return torch.full(shape, -1, dtype=torch.int32, device=torch.device(DEV))


def mask_dev(mask):
    import torch
    return None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).to(torch.device(DEV))


def chain(rsv, ctx, wp, batch, inputs, b, upto="commit", caps=False, log_last=None, by_variable=False, outputs=None):
    """rsv.Chain on a batch with the tests' prefill, run through the stage `upto`; outputs: Chain.trace()'s keywords."""
    ch = rsv.Chain(ctx, wp, len(batch), b, log_last=log_last, fill=FILL, caps=caps, device=DEV)
    ch.witness(batch, inputs, by_variable=by_variable)
    for stage in STAGES[1:STAGES.index(upto) + 1]:
        getattr(ch, stage)(**(outputs or {}) if stage == "trace" else {})
    return ch


def tail(ch, cfg, distinct=False):
    """Proof of work, queries and openings of a chain that has run through fri().  distinct (one proof): the smallest nonce
    whose queries are distinct at the largest column's size.  The verifier rejects a proof with a duplicate there
    (RSV_R_DUP_QUERY, as the reference's answer gadget does), and on 2^11 positions 128 queries have one 98 times in a
    hundred."""
    if distinct:
        assert ch.n == 1
        ch.ctx.synchronize()
        before = ch.channel.clone()
    start = 0
    for _ in range(1 << 14):
        ch.pow(cfg.pow_bits, cfg.n_queries, start=start)
        if not distinct:
            break
        ch.ctx.synchronize()
        q = ch.queries.cpu().numpy().view(np.uint32)[0].tolist()
        if not ch.ok.cpu().tolist()[0] or len(set(q)) == len(q):
            break
        lo, hi = ch.nonce.cpu().numpy().view(np.uint32)[0].tolist()
        start = (hi << 32 | lo) + 1
        ch.channel.copy_(before)
    else:
        raise AssertionError("no nonce with distinct queries")
    ch.open()
    ch.fri_open()
    return ch


def whole_chain(rsv, ctx, wp, batch, inputs, cfg, caps=True, distinct=False):
    """The whole chain of a batch under the configuration cfg -> (Chain.numpy(), Chain.proofs()); distinct: tail()'s."""
    ch = chain(rsv, ctx, wp, batch, inputs, cfg.log_blowup_factor, upto="fri", caps=caps, log_last=cfg.log_last_layer_degree_bound)
    tail(ch, cfg, distinct)
    return ch.numpy(), ch.proofs()


def slots_differ(got, k, want, j):
    """The tensors of two Chain.numpy() results in which slot k of `got` is not word for word slot j of `want`."""
    assert set(got) == set(want)
    return [key for key in got if not np.array_equal(got[key][k], want[key][j])]


def masked_past_64(n=70):
    """The mask of a batch past one 64-lane workgroup of proofs: the last lane of the first workgroup and the first of the
    second are cleared."""
    return [0 if p in (63, 64) else 1 for p in range(n)]
