"""tests/pow_ref.py pinned to the reference on one fixture, without a device: from the channel rebuilt from the proof's own
transcript values, the smallest qualifying nonce counted from 0 is the proof's stored nonce, the digest behind its mix is the
oracle's proof-of-work digest, and the draws that follow give the oracle's query positions; the new entry points are
exported."""
import numpy as np

from tests import commit_ref as C
from tests import oracle_binding as ob
from tests import pow_ref as W
from tests.conftest import fixture_cfg, read_proof

FIXTURE = "level7-1.bin"


def test_restatement_gives_the_fixtures_nonce_and_queries():
    proof = read_proof(FIXTURE)
    cfg = fixture_cfg(FIXTURE)
    tr = ob.transcript_raw(proof)
    chan = W.channel_before_pow(proof, ob)
    assert W.stored_nonce(proof, ob) == 158323
    assert W.grind(chan, cfg.pow_bits, 0, 1 << 26, ob) == 158323
    assert W.grind(chan, cfg.pow_bits, 0, 158323, ob) is None
    after = W.mix_nonce(chan, 158323, ob)
    assert np.array_equal(after[:8], tr[32:40].astype(np.uint32)) and not after[8:].any()
    qM, M = C.query_positions(proof, ob)
    lay = ob.proof_layout(proof)
    low = max(lay["lp"], lay["lq"]) + cfg.log_blowup_factor
    q, q_low, behind = W.draw_queries(after, cfg.n_queries, M, low, ob)
    assert np.array_equal(q.astype(np.int64), qM)
    assert np.array_equal(q_low.astype(np.int64), qM >> (M - low))
    assert behind[8] == (cfg.n_queries + 7) // 8 and np.array_equal(behind[:8], after[:8])


def test_nonce_words_cross_the_boundaries():
    w = W.nonce_words(np.array([(1 << 22) - 1, 1 << 22, (1 << 43) - 1, 1 << 43, (1 << 64) - 1], dtype=np.uint64))
    assert [int(x) for x in w[0]] == [(1 << 22) - 1, 0, (1 << 22) - 1, 0, (1 << 22) - 1]
    assert [int(x) for x in w[1]] == [0, 1, (1 << 21) - 1, 0, (1 << 21) - 1]
    assert [int(x) for x in w[2]] == [0, 0, 0, 1, (1 << 21) - 1]


def test_entry_points_are_exported(rsv):
    for name in ("rsv_pow_grind_dev", "rsv_draw_queries_dev"):
        assert name in rsv.EXPORTS and hasattr(rsv.lib, name)
    assert hasattr(rsv.Context, "pow_grind") and hasattr(rsv.Context, "draw_queries")
    assert hasattr(rsv.Chain, "pow") and hasattr(rsv.Chain, "open")
