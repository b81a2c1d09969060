"""GPU: the permutation entered through centre_rc (the sign-mask select of the S-box input, poseidon2.hpp) against the oracle.

rsv_poseidon2_permute_dev (the paced out-of-line instance) runs 2^16 random states plus states built to put the select's
operand a = t - c on both sides of zero: first-round a equal to -2, -1, 0, 1 and -c in all 16 words at once (the external
matrix is inverted mod P on the CPU model of tests/perm_model.py, which also confirms each a), and every word in turn
at 0 and P - 1.  The unpaced instances are reached through a small batch's verify (at most 1 024 proofs)."""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import perm_model as pm
from tests.conftest import fixture_cfg, read_proof

pytestmark = pytest.mark.gpu

P = 0x7FFFFFFF


def _matrix(model):
    """the external matrix mod P, from the model's doubled linear layer on unit vectors"""
    cols = [[(v // 2) % P for v in model.mds16_2x([1 if i == j else 0 for i in range(16)])] for j in range(16)]
    return [[cols[j][i] for j in range(16)] for i in range(16)]


def _solve(M, y):
    """s with M s = y mod P (Gauss-Jordan over the field)"""
    n = len(y)
    A = [row[:] + [v % P] for row, v in zip(M, y)]
    for k in range(n):
        p = next(r for r in range(k, n) if A[r][k] % P)
        A[k], A[p] = A[p], A[k]
        inv = pow(A[k][k], P - 2, P)
        A[k] = [v * inv % P for v in A[k]]
        for r in range(n):
            if r != k and A[r][k]:
                f = A[r][k]
                A[r] = [(a - f * b) % P for a, b in zip(A[r], A[k])]
    return [A[i][n] for i in range(n)]


def _first_round_a(model, st):
    full, _ = pm.constants()
    V = model.mds16_2x(st)
    return [model.fold2(V[i]) - (P - pm.centred(full[0][i])) for i in range(16)]


def _edge_states():
    model = pm.model(pm.Exact)
    full, _ = pm.constants()
    M = _matrix(model)
    c = [P - pm.centred(rc) for rc in full[0]]
    states = []
    for k in (-2, -1, 0, 1):
        st = _solve(M, [ci + k for ci in c])
        assert _first_round_a(model, st) == [k] * 16, k          # the fold lands on c + k itself, not on c + k + P
        states.append(st)
    assert _first_round_a(model, [0] * 16) == [-ci for ci in c]
    states.append([0] * 16)
    # one word at a time on either side, the others at the a = -1 / a = 0 states
    for i in range(16):
        y_neg, y_pos = [ci for ci in c], [ci - 1 for ci in c]
        y_neg[i], y_pos[i] = c[i] - 1, c[i]
        for y in (y_neg, y_pos):
            st = _solve(M, y)
            a = _first_round_a(model, st)
            assert a == [v - ci for v, ci in zip(y, c)]
            states.append(st)
        # t congruent to 0 in word i alone: the fold of a non-zero multiple of P is P itself, so a is P - c, the far
        # positive end (a = -c needs t = 0, the all-zero state above)
        y_zero = [ci for ci in c]
        y_zero[i] = 0
        st = _solve(M, y_zero)
        assert _first_round_a(model, st)[i] in (-c[i], P - c[i])
        states.append(st)
    rng = np.random.default_rng(163)
    for i in range(16):
        for v in (0, P - 1):
            st = [int(w) for w in rng.integers(0, P, 16)]
            st[i] = v
            states.append(st)
    states += [[P - 1] * 16, [P - 1 if i % 2 else 0 for i in range(16)]]
    return np.array(states, dtype=np.uint32)


def _permute_dev(rsv, s):
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(s.view(np.int32)).to(dev)
    d_out = torch.empty_like(d_in)
    d_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx = rsv.Context(0)
    ctx.poseidon2_permute(d_in, d_out, d_bad)
    ctx.synchronize()
    assert int(d_bad.item()) == 0
    return d_out.cpu().numpy().view(np.uint32)


def test_permute_dev_random_states(rsv):
    rng = np.random.default_rng(164)
    s = rng.integers(0, P, (1 << 16, 16), dtype=np.uint32)
    assert np.array_equal(_permute_dev(rsv, s), ob.poseidon2_permute(s))


def test_permute_dev_select_edges(rsv):
    s = _edge_states()
    assert s.max() <= P - 1
    want = ob.poseidon2_permute(s)
    assert np.array_equal(_permute_dev(rsv, s), want)
    assert np.array_equal(rsv.poseidon2_permute(s), want)


def test_unpaced_instances_through_a_small_batch(rsv):
    """A batch of at most 1 024 proofs hashes its trees with the unpaced instances: verdicts and reasons equal the oracle's."""
    proof = read_proof("recursive_proof_16_15.bin")
    batch = [proof] + [ob.tamper(proof, i) for i in range(15)]
    cfgs = [fixture_cfg("recursive_proof_16_15.bin")] * 16
    acc, reason = rsv.verify_batch(batch, cfgs)
    oacc, oreason = ob.verify_batch(batch, cfgs)
    assert acc.tolist() == oacc.tolist() and reason.tolist() == oreason.tolist()
    assert acc[0] == 1 and acc[1:].sum() == 0
