"""GPU: the permutation with the external layer's column sums formed first (PermT::colsums_2x / mds_group_2x and the
half-output tail, poseidon2.hpp) against the oracle.

rsv_poseidon2_permute_dev (the paced out-of-line instance with the whole output state) runs 2^12 states: the all-zero
state, all words at P - 1, each word alone at P - 1, the rest random.  The four half-output instances are reached through
verify: a 16-proof batch hashes its trees with the unpaced rate and capacity instances, a 2 048-proof batch with the paced
ones (verify_api.inc picks the form by batch size); these are the smallest batches that reach each."""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu

P = 0x7FFFFFFF
NAME = "recursive_proof_16_15.bin"


def test_permute_dev_equals_the_oracle(rsv):
    import torch
    rng = np.random.default_rng(191)
    s = rng.integers(0, P, (1 << 12, 16), dtype=np.uint32)
    s[0] = 0
    s[1] = P - 1
    s[2:18] = 0
    s[np.arange(2, 18), np.arange(16)] = P - 1
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(s.view(np.int32)).to(dev)
    d_out = torch.empty_like(d_in)
    d_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx = rsv.Context(0)
    ctx.poseidon2_permute(d_in, d_out, d_bad)
    ctx.synchronize()
    assert int(d_bad.item()) == 0
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), ob.poseidon2_permute(s))
    ctx.close()


def test_unpaced_half_instances_through_sixteen_proofs(rsv):
    proof = read_proof(NAME)
    batch = [proof] * 15 + [ob.tamper(proof, 5)]
    cfgs = [fixture_cfg(NAME)] * 16
    acc, reason = rsv.verify_batch(batch, cfgs)
    oacc, oreason = ob.verify_batch(batch[-2:], cfgs[-2:])
    assert acc.tolist() == [int(oacc[0])] * 15 + [int(oacc[1])] and reason.tolist() == [int(oreason[0])] * 15 + [int(oreason[1])]
    assert acc.tolist() == [1] * 15 + [0]


def test_paced_half_instances_through_2048_proofs(rsv):
    """128 copies of eight genuine and eight differently tampered proofs: the oracle verifies each distinct proof once."""
    proof = read_proof(NAME)
    tile = [proof] * 8 + [ob.tamper(proof, i) for i in range(8)]
    oacc, oreason = ob.verify_batch(tile[7:], [fixture_cfg(NAME)] * 9)
    want_acc = ([int(oacc[0])] * 8 + oacc[1:].tolist()) * 128
    want_reason = ([int(oreason[0])] * 8 + oreason[1:].tolist()) * 128
    acc, reason = rsv.verify_batch(tile * 128, [fixture_cfg(NAME)] * 2048)
    assert acc.tolist() == want_acc and reason.tolist() == want_reason
    assert sum(want_acc) == 8 * 128
