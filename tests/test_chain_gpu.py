"""rsv.Chain (`-m gpu`): the chain's buffers and stages as one object.  One proof of the level2-1.bin pair at that pair's own
blowup: every tensor a Chain run through fri() holds equals, word for word, what the same Context.witness_* calls write
into tensors allocated here by hand (the one place that still spells those calls out), every output prefilled with
0xffffffff; and a stage called before the one it depends on raises ValueError with nothing enqueued."""
import numpy as np
import pytest

from tests.chain_harness import DEV, chain, dev, full, inputs_of, pin_of, program_of
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
SRC = "level2-1.bin"


def _loose(rsv, ctx, wp, proof, inputs, b, log_last, queries):
    """The chain as loose Context calls on tensors of its own -> dict of the tensors, named as Chain's attributes."""
    import torch
    n = 1
    lp, lq = wp.trace_sizes()
    F = wp.shape.flow_count
    n_ops = len(wp.gates()[1])
    flag = lambda v: torch.full((n,), v, dtype=torch.uint8, device=DEV)  # noqa: E731
    blob, offsets = rsv.pack([proof])
    d_blob, d_off = torch.from_numpy(blob.copy()).to(DEV), torch.from_numpy(offsets.astype(np.int64)).to(DEV)
    d_vars = torch.zeros((n, wp.n_vars, 4), dtype=torch.int32, device=DEV)
    d_flow = torch.zeros((n, F, 32), dtype=torch.int32, device=DEV)
    d_swap = torch.zeros((n, F), dtype=torch.uint8, device=DEV)
    t = {"acc": flag(0)}
    ctx.witness(wp, d_blob, d_off, n, d_vars, t["acc"], inputs=inputs, d_flow=d_flow, d_flow_swap=d_swap)
    t.update(plonk=full((n, 12, 1 << lp)), poseidon=full((n, 48, 1 << lq)), ops=full((n, max(n_ops, 1))))
    ctx.witness_trace(wp, d_vars, t["acc"], n, d_plonk=t["plonk"], d_poseidon=t["poseidon"], d_ops=t["ops"], d_flow=d_flow, d_flow_swap=d_swap)
    t.update(roots=full((n, 3, 8)), draws=full((n, 12)), int_plonk=full((n, 8, 1 << lp)), int_poseidon=full((n, 8, 1 << lq)),
             sums=full((n, 2, 4)), channel=full((n, 16)), ok=flag(7), caps=full((n, 3, 2 << b, 8)))
    ctx.witness_commit(wp, t["plonk"], t["poseidon"], t["ops"], t["acc"], n, b, t["roots"], t["draws"], t["int_plonk"], t["int_poseidon"],
                       t["sums"], d_channel=t["channel"], d_ok=t["ok"], d_caps=t["caps"])
    vcaps, wcap = rsv.witness_decommit_sizes(wp, b, queries.shape[1])
    d_q = dev(queries)  # held to the end: the opening reads it on the context's stream
    t.update(values=full((n, sum(vcaps))), n_values=full((n, 3)), witness=full((n, 3, wcap, 8)), n_witness=full((n, 3)))
    ctx.witness_decommit(wp, t["plonk"], t["poseidon"], t["ops"], t["int_plonk"], t["int_poseidon"], t["acc"], n, b, d_q,
                         queries.shape[1], t["values"], t["n_values"], t["witness"], t["n_witness"], d_ok=t["ok"], d_caps=t["caps"])
    L3 = rsv.composition_log_size(lp, lq)
    t.update(comp=full((n, 8, 1 << L3)), root3=full((n, 8)), oods=full((n, 8)), samples3=full((n, 8, 4)), cap3=full((n, 2 << b, 8)))
    ctx.witness_tree3(wp, t["plonk"], t["poseidon"], t["ops"], t["int_plonk"], t["int_poseidon"], t["acc"], n, b, t["sums"], t["draws"],
                      t["channel"], t["comp"], t["root3"], t["oods"], t["samples3"], d_ok=t["ok"], d_cap3=t["cap3"])
    t["samples"] = full((n, 134, 4))
    ctx.witness_sample(wp, t["plonk"], t["poseidon"], t["ops"], t["int_plonk"], t["int_poseidon"], t["acc"], n, t["oods"], t["samples"],
                       d_ok=t["ok"])
    sz = rsv.fri_sizes(lp, lq, b, log_last)
    ni = sz["n_inner"]
    t.update(after=full((n, 4)), quot=full((n, sz["quot_words"])), fri_roots=full((n, 1 + ni, 8)), alphas=full((n, 1 + ni, 4)),
             layers=full((n, max(sz["layer_words"], 1))), last_poly=full((n, 1 << log_last, 4)), low_degree=flag(7))
    ctx.witness_fri(wp, t["plonk"], t["poseidon"], t["ops"], t["int_plonk"], t["int_poseidon"], t["acc"], n, b, log_last, t["comp"], t["oods"],
                    t["samples"], t["samples3"], t["channel"], t["after"], t["quot"], t["fri_roots"], t["alphas"], t["layers"], t["last_poly"],
                    t["low_degree"], d_ok=t["ok"])
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["ops"] = out["ops"][:, :n_ops]
    return {k: v if v.dtype == np.uint8 else v.view(np.uint32) for k, v in out.items()}


def test_chain_writes_the_words_of_the_loose_calls(rsv):
    pin = pin_of(SRC)
    wp = program_of(rsv, pin)
    cfg = fixture_cfg(pin["dst"])
    b, log_last = cfg.log_blowup_factor, cfg.log_last_layer_degree_bound
    top = max(wp.trace_sizes()) + b
    queries = np.random.default_rng(26).integers(0, 1 << top, (1, 5)).astype(np.uint32)
    ctx = rsv.Context(0)
    want = _loose(rsv, ctx, wp, read_proof(SRC), inputs_of(SRC), b, log_last, queries)
    ch = chain(rsv, ctx, wp, [read_proof(SRC)], inputs_of(SRC), b, upto="commit", caps=True, log_last=log_last)
    opened = {k: full(want[k].shape) for k in ("values", "n_values", "witness", "n_witness")}
    d_q = dev(queries)  # held to the end: the opening reads it on the context's stream
    ch.decommit(d_q, opened["values"], opened["n_values"], opened["witness"], opened["n_witness"])
    ch.tree3()
    ch.sample()
    ch.fri()
    got = ch.numpy()
    got.update({k: v.cpu().numpy().view(np.uint32) for k, v in opened.items()})
    ctx.close()
    wp.close()
    assert got["acc"].tolist() == [1] and got["ok"].tolist() == [1] and got["low_degree"].tolist() == [1]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_a_stage_before_the_one_it_needs_is_refused(rsv):
    """fri() before tree3(), tree3() before commit() and fri() on a chain that lacks only sample() raise ValueError naming
    the missing stage; nothing is enqueued and nothing allocated: the tensors of the stages that ran are unchanged (tree 3's
    channel among them, which fri() would move on), the refused stage's are still None."""
    pin = pin_of(SRC)
    wp = program_of(rsv, pin)
    cfg = fixture_cfg(pin["dst"])
    ctx = rsv.Context(0)
    ch = chain(rsv, ctx, wp, [read_proof(SRC)], inputs_of(SRC), cfg.log_blowup_factor, upto="trace", log_last=cfg.log_last_layer_degree_bound)
    before = ch.numpy()
    with pytest.raises(ValueError, match="commit"):
        ch.tree3()
    assert ch.comp is None and ch.roots is None and ch.done == {"trace"}
    ch.commit()
    after_commit = ch.numpy()
    with pytest.raises(ValueError, match="tree3"):
        ch.fri()
    with pytest.raises(ValueError, match="tree3"):
        ch.sample()
    assert ch.quot is None and ch.samples is None and ch.comp is None
    now = ch.numpy()
    ch.tree3()
    after_tree3 = ch.numpy()
    with pytest.raises(ValueError, match="sample"):
        ch.fri()
    assert ch.quot is None and ch.samples is None and ch.done == {"trace", "commit", "tree3"}
    last = ch.numpy()
    ctx.close()
    wp.close()
    assert sorted(now) == sorted(after_commit) and all(np.array_equal(now[k], after_commit[k]) for k in now)
    assert all(np.array_equal(now[k], before[k]) for k in before)
    assert now["ok"].tolist() == [1]
    assert sorted(last) == sorted(after_tree3) and all(np.array_equal(last[k], after_tree3[k]) for k in last)
    assert not (last["comp"] == 0xFFFFFFFF).all() and last["ok"].tolist() == [1]
