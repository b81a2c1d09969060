"""The next-proof chain on batches whose proofs differ (`-m gpu`).  Every other chain-level batch in the suite is k copies of
one fixture, so its live slots are bit-identical and a p-for-p0 + p slip, a read of slot 0's per-proof data or a wrong proof
stride in a wrapper passes there.  Here the batches mix A = level10-1.bin and B = level11-1.bin under A's program (which
accepts both, tests/test_witness_gpu.py) with a tampered A among them: the slot of A is pinned to the REFERENCE (the next
fixture's file, byte for byte), the slots of B to their solo run and to the two verifiers (the C oracle and the library's own:
a serialised proof is accepted only if every root, draw, sample, nonce, query and opening in it belongs to that proof), once at
the pair's own configuration, once with every driver cut to one proof per pass, once past one 64-lane workgroup of proofs.
Every comparison is exact on 32-bit words; outputs are prefilled with 0xffffffff."""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests.chain_harness import inputs_of, pin_of, program_of, slots_differ, whole_chain
from tests.conftest import Cfg, fixture_cfg, read_proof

pytestmark = pytest.mark.gpu
A, B = "level10-1.bin", "level11-1.bin"


@pytest.fixture(scope="module")
def wp(rsv):
    prog = program_of(rsv, pin_of(A))
    yield prog
    prog.close()


def _kinds():
    a, b = read_proof(A), read_proof(B)
    return {"A": a, "B": b, "bad": ob.tamper(a, 5)}


def _run(rsv, ctx, wp, kinds, cfg):
    proofs = _kinds()
    return whole_chain(rsv, ctx, wp, [proofs[k] for k in kinds], inputs_of(A), cfg)


def _zero_slot(got, proofs, p):
    assert proofs[p] is None
    assert [key for key in got if got[key][p].any()] == [], p


def _check_slots(kinds, got, proofs, solo):
    """Every live slot of a batch is its kind's solo run in every tensor and in its bytes; a rejected slot is zero / None."""
    assert got["ok"].tolist() == [0 if k == "bad" else 1 for k in kinds]
    for p, kind in enumerate(kinds):
        if kind == "bad":
            _zero_slot(got, proofs, p)
            continue
        want, want_bytes = solo[kind]
        assert slots_differ(got, p, want, 0) == [], (p, kind)
        assert proofs[p] == want_bytes[0], (p, kind)


def _check_accepted(rsv, proofs, cfg):
    """The C oracle (oracle/rsv_oracle.c, independent of the library) and the library's verifier accept these bytes."""
    for verify in (ob.verify_batch, rsv.verify_batch):
        acc, reason = verify(proofs, cfg, inputs_of(B))
        assert acc.tolist() == [1] * len(proofs) and reason.tolist() == [0] * len(proofs), (verify.__module__, acc.tolist(), reason.tolist())


def test_heterogeneous_batch_is_pinned_to_the_reference(rsv, wp):
    """[B, A, tamper(A), B] at level11-1.bin's own configuration (pow_bits 20, b = 8, log_last 8, 10 queries), with the caps.
    A sits in slot 1, so that "everyone gets slot 0's values" breaks the slot the reference pins: its bytes are
    level11-1.bin's.  The two B slots are equal to each other and to the solo run [B] in every tensor, the rejected slot is
    zero, and both verifiers accept the B slots' bytes.  The batch is heterogeneous where the per-proof code is: the op
    column (k_cm_op_patch: tree 0 itself is per-proof), the roots of trees 0 and 1, the draws, the OODS point, `after`, the
    nonce, the queries and the witness counts differ between slots 0 and 1."""
    cfg = fixture_cfg(B)
    assert (cfg.pow_bits, cfg.log_blowup_factor, cfg.log_last_layer_degree_bound, cfg.n_queries) == (20, 8, 8, 10)
    kinds = ["B", "A", "bad", "B"]
    ctx = rsv.Context(0)
    got, proofs = _run(rsv, ctx, wp, kinds, cfg)
    solo, solo_proofs = _run(rsv, ctx, wp, ["B"], cfg)
    ctx.close()
    assert got["ok"].tolist() == [1, 1, 0, 1]
    want = read_proof(B)
    assert len(proofs[1]) == len(want) and proofs[1] == want
    assert slots_differ(got, 0, got, 3) == []
    for p in (0, 3):
        assert slots_differ(got, p, solo, 0) == [], p
        assert proofs[p] == solo_proofs[0], p
    _zero_slot(got, proofs, 2)
    _check_accepted(rsv, [proofs[0], proofs[3]], cfg)
    # without this the test says nothing about k_cm_op_patch: the op column must differ between the two kinds
    assert not np.array_equal(got["ops"][0], got["ops"][1]), "the op columns of level10-1.bin and level11-1.bin are equal: the batch is not heterogeneous"
    differ = set(slots_differ(got, 0, got, 1))
    assert {"ops", "draws", "oods", "after", "nonce", "queries"} <= differ, differ
    assert not np.array_equal(got["roots"][0, 0], got["roots"][1, 0]) and not np.array_equal(got["roots"][0, 1], got["roots"][1, 1])
    assert differ & {"n_witness", "n_fri_hash_witness"}, differ


def test_one_proof_per_pass_equals_the_uncut_batch(rsv, wp):
    """[B, A, tamper(A), B, A] at pow_bits 20, b = 1, log_last 8, 10 queries, once at the default workspace budget and once
    under 1 MB, set before the witness.  plan_pass never refuses: it halves the blocks to one, then the proofs to one, and
    runs.  At 2^16 / 2^15 rows the workspace of two proofs exceeds 1 MB in every driver, by one part alone:
      commit, decommit and sample of trees 0-2: the coefficients of the tree's Plonk columns of 2^16 words (3, 12 and 8 of
        them: the first group of each tree, held per proof whether shared or not);
      composition and the quotients' pass of size lp: the coefficients of the 12 Plonk trace columns;
      the quotients' pass of size lq: those of the 48 Poseidon trace columns of 2^15 words;
      the quotients' pass of size L3, and tree 3's sample and decommit: those of the composition's 8 columns of 2^17 words;
      fri_commit and fri_open: two node layers of 48 x 2^M bytes, M = 18.
    So every pass is one proof and every slot is reached at its own p0.  Every tensor of the cut run equals the uncut run's,
    the uncut slots their solo runs, and both verifiers accept the four live slots' bytes."""
    cfg = Cfg(20, 1, 8, 10)
    budget = 1 << 20
    lp, lq = wp.trace_sizes()
    L3, M = rsv.composition_log_size(lp, lq), rsv.fri_sizes(lp, lq, 1, 8)["sizes"][0]
    assert (lp, lq, L3, M) == (16, 15, 17, 18)
    for cols, log in ((3, lp), (12, lp), (8, lp), (48, lq), (8, L3)):
        assert 2 * 4 * (cols << log) > budget, (cols, log)
    assert 2 * (48 << M) > budget
    kinds = ["B", "A", "bad", "B", "A"]
    ctx = rsv.Context(0)
    whole, whole_proofs = _run(rsv, ctx, wp, kinds, cfg)
    solo = {k: _run(rsv, ctx, wp, [k], cfg) for k in ("A", "B")}
    ctx.close()
    ctx = rsv.Context(0)
    ctx.set_option("ws_budget_mb", 1)
    cut, cut_proofs = _run(rsv, ctx, wp, kinds, cfg)
    ctx.close()
    assert [key for key in whole if not np.array_equal(cut[key], whole[key])] == []
    assert cut_proofs == whole_proofs
    _check_slots(kinds, whole, whole_proofs, solo)
    _check_accepted(rsv, [p for p in whole_proofs if p is not None], cfg)


def test_past_one_workgroup_of_proofs(rsv, wp):
    """67 proofs, slot k A where k % 3 == 0 and B elsewhere, slots 63 and 65 tamper(A), at pow_bits 12, b = 1, log_last 8, 10
    queries: the kernels that index p = blockIdx.x * 64 + threadIdx.x run a second workgroup; one rejected proof is the last
    lane of the first workgroup, the other sits inside the second.  Every live slot is its kind's solo run in every tensor
    and in its bytes, the rejected ones are zero, and the C oracle accepts one slot of each kind on each side of the
    workgroup boundary."""
    cfg = Cfg(12, 1, 8, 10)
    kinds = ["bad" if k in (63, 65) else "A" if k % 3 == 0 else "B" for k in range(67)]
    assert [kinds[k] for k in (0, 62, 64, 66)] == ["A", "B", "B", "A"]
    ctx = rsv.Context(0)
    got, proofs = _run(rsv, ctx, wp, kinds, cfg)
    solo = {k: _run(rsv, ctx, wp, [k], cfg) for k in ("A", "B")}
    ctx.close()
    assert got["ok"].shape == (67,) and (got["ok"] == 0).sum() == 2
    _check_slots(kinds, got, proofs, solo)
    acc, reason = ob.verify_batch([proofs[k] for k in (0, 62, 64, 66)], cfg, inputs_of(B))
    assert acc.tolist() == [1, 1, 1, 1] and reason.tolist() == [0, 0, 0, 0]
