"""Chain.proofs (`-m gpu`): the serialised proof of the next recursion level.  For all 14 consecutive fixture pairs the chain of
fixture K, given K+1's configuration and nothing else of it, puts out K+1's file byte for byte, and the library's own
verifier accepts those bytes under K+1's configuration and public inputs; a batch with a tampered middle proof gives None
there and its neighbours' bytes unchanged."""
import pytest

from tests import oracle_binding as ob
from tests.chain_harness import chain, inputs_of, pin_id, pin_of, pins, program_of
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu


def _proofs(rsv, pin, batch):
    src, cfg = pin["src"], fixture_cfg(pin["dst"])
    wp = program_of(rsv, pin)
    ctx = rsv.Context(0)
    ch = chain(rsv, ctx, wp, batch, inputs_of(src), cfg.log_blowup_factor, upto="fri", caps=True, log_last=cfg.log_last_layer_degree_bound)
    with pytest.raises(ValueError):
        ch.proofs()  # needs open() and fri_open() first
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.open()
    ch.fri_open()
    out = ch.proofs()
    ctx.close()
    wp.close()
    return out


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_chain_of_fixture_k_outputs_fixture_k_plus_1(rsv, pin):
    dst = pin["dst"]
    got = _proofs(rsv, pin, [read_proof(pin["src"])])
    want = read_proof(dst)
    assert len(got) == 1 and got[0] is not None
    assert len(got[0]) == len(want), (len(got[0]), len(want))
    assert got[0] == want
    acc, reason = rsv.verify_batch(got, fixture_cfg(dst), inputs_of(dst))
    assert acc.tolist() == [1] and reason.tolist() == [0]


def test_batch_with_a_tampered_middle_proof(rsv):
    pin = pin_of("level2-1.bin")
    proof = read_proof(pin["src"])
    got = _proofs(rsv, pin, [proof, ob.tamper(proof, 5), proof])
    want = read_proof(pin["dst"])
    assert got[1] is None and got[0] == want and got[2] == want
