"""Per-proof public inputs, what shows without a device: the refusals of the new entry points (before any device work,
in the manner of tests/test_user_circuit_host.py), the Python-integer model of the statement sum against the oracle's
field operations, and the model of the kernel's batched inversion against the per-term model with zero denominators at
the first, a middle and the last position of a chunk."""
import ctypes

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import user_circuit_ref as U
from tests import verify_inputs_ref as V

NULL, SIZE, RANGE = -1, -2, -5
P = V.P
u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)


def test_refusals_come_before_any_device_work(rsv):
    lib = rsv.lib
    one = ctypes.c_void_p(16)   # non-NULL, 16-byte aligned, never dereferenced: the refusal comes first
    odd = ctypes.c_void_p(18)   # not 4-byte aligned
    cfg = rsv.prepare_cfg(rsv.PcsConfig(20, 5, 8, 16), 1)
    ho = rsv.HintsOut()
    # rsv_verify_batch_inputs_dev / rsv_verify_hints_inputs_dev
    for call in (lambda *a: lib.rsv_verify_batch_inputs_dev(*a[:7], one, None),
                 lambda *a: lib.rsv_verify_hints_inputs_dev(*a[:7], ctypes.byref(ho), one, None)):
        assert call(None, one, one, 1, cfg.ref(), one, 3) == NULL                 # no context
        assert call(one, one, one, 1, cfg.ref(), None, 3) == NULL                 # inputs missing
        assert call(one, None, one, 1, cfg.ref(), one, 3) == NULL                 # blob missing
        assert call(one, one, one, 1, None, one, 3) == NULL                       # the configuration is required
        assert call(one, one, one, 1, cfg.ref(), one, 4097) == SIZE               # n_pi > 4096
        assert call(one, one, one, (1 << 20) + 1, cfg.ref(), one, 1024) == SIZE   # n * n_pi > RSV_MAX_INPUT_RECORDS = 2^30
        assert call(one, one, one, 1 << 27, cfg.ref(), None, 0) == SIZE           # n beyond rsv_verify_batch_dev's own bound
        assert call(one, one, one, 1, cfg.ref(), odd, 3) == SIZE                  # alignment
        assert call(one, one, one, 0, cfg.ref(), None, 0) == 0                    # an empty batch, d_pi NULL with n_pi = 0
    assert lib.rsv_verify_hints_inputs_dev(one, one, one, 1, cfg.ref(), one, 3, None, one, None) == NULL
    # rsv_public_input_sum_dev
    assert lib.rsv_public_input_sum_dev(None, one, 1, 3, one, one, None) == NULL
    assert lib.rsv_public_input_sum_dev(one, None, 1, 3, one, one, None) == NULL
    assert lib.rsv_public_input_sum_dev(one, one, 1, 3, None, one, None) == NULL
    assert lib.rsv_public_input_sum_dev(one, one, 1, 3, one, None, None) == NULL
    assert lib.rsv_public_input_sum_dev(one, one, 1, 4097, one, one, None) == SIZE
    assert lib.rsv_public_input_sum_dev(one, one, (1 << 18) + 1, 4096, one, one, None) == SIZE
    assert lib.rsv_public_input_sum_dev(one, one, (1 << 26) + 1, 1, one, one, None) == SIZE
    assert lib.rsv_public_input_sum_dev(one, odd, 1, 3, one, one, None) == SIZE
    assert lib.rsv_public_input_sum_dev(one, None, 0, 0, None, None, None) == 0
    # rsv_verify_batch_inputs: host records are checked on the host, as the shared form's
    blob, offsets = rsv.pack([b"\0" * 64, b"\0" * 64])
    acc = np.zeros(2, np.uint8)
    lead = (blob.ctypes.data_as(u8p), offsets.ctypes.data_as(u64p), 2)
    cfg2 = rsv.prepare_cfg(rsv.PcsConfig(20, 5, 8, 16), 2)
    good = [[(1, (1, 0, 0, 0)), (2, (5, 6, 7, 8))], [(1, (1, 0, 0, 0)), (2, (P - 1, 0, 0, 0))]]
    pi, n_pi = rsv.make_inputs_per_proof(good, 2)
    a8 = acc.ctypes.data_as(u8p)
    assert lib.rsv_verify_batch_inputs(*lead, cfg2.ref(), None, 2, a8, None, 0) == NULL
    assert lib.rsv_verify_batch_inputs(*lead, cfg2.ref(), pi, n_pi, None, None, 0) == NULL
    assert lib.rsv_verify_batch_inputs(*lead, None, pi, n_pi, a8, None, 0) == NULL
    assert lib.rsv_verify_batch_inputs(*lead, cfg2.ref(), pi, 4097, a8, None, 0) == SIZE
    bad = [good[0], [(1, (1, 0, 0, 0)), (2, (0, 0, P, 0))]]                      # proof 1, input 1, word 2 = P
    pi_bad, _ = rsv.make_inputs_per_proof(bad, 2)
    assert lib.rsv_verify_batch_inputs(*lead, cfg2.ref(), pi_bad, 2, a8, None, 0) == RANGE
    with pytest.raises(rsv.RsvError) as e:
        rsv.verify_batch([b"\0" * 64] * 2, rsv.PcsConfig(20, 5, 8, 16), inputs_per_proof=bad)
    assert e.value.code == RANGE
    with pytest.raises(ValueError):
        rsv.verify_batch([b"\0" * 64] * 2, rsv.PcsConfig(20, 5, 8, 16), inputs_per_proof=[good[0], good[1][:1]])
    with pytest.raises(ValueError):
        rsv.verify_batch([b"\0" * 64] * 2, rsv.PcsConfig(20, 5, 8, 16), inputs_per_proof=good[:1])
    assert rsv.inputs_array(good, 2).tolist() == [[[1, 1, 0, 0, 0], [2, 5, 6, 7, 8]], [[1, 1, 0, 0, 0], [2, P - 1, 0, 0, 0]]]


def test_circuit_inputs_refusals_and_num_input(rsv):
    b = U.build("S1")
    c = rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, b.witness_ops)
    lib, one, out = rsv.lib, ctypes.c_void_p(16), ctypes.c_uint32(0)
    assert lib.rsv_circuit_program_num_input(c._h, ctypes.byref(out)) == 0 and out.value == b.num_input == 4
    assert lib.rsv_circuit_program_num_input(None, ctypes.byref(out)) == NULL
    assert lib.rsv_circuit_program_num_input(c._h, None) == NULL
    assert lib.rsv_circuit_inputs_dev(None, c._h, one, 1, one) == NULL
    assert lib.rsv_circuit_inputs_dev(one, None, one, 1, one) == NULL
    assert lib.rsv_circuit_inputs_dev(one, c._h, None, 1, one) == NULL
    assert lib.rsv_circuit_inputs_dev(one, c._h, one, 1, None) == NULL
    assert lib.rsv_circuit_inputs_dev(one, c._h, one, (1 << 20) + 1, one) == SIZE
    assert lib.rsv_circuit_inputs_dev(one, c._h, ctypes.c_void_p(20), 1, one) == SIZE    # d_variables not 16-byte aligned
    assert lib.rsv_circuit_inputs_dev(one, c._h, one, 1, ctypes.c_void_p(18)) == SIZE
    c.close()


def test_field_model_is_the_oracles():
    rnd = np.random.default_rng(7)
    for _ in range(40):
        a, b = (tuple(int(x) for x in rnd.integers(0, P, 4)) for _ in range(2))
        assert list(V.q_mul(a, b)) == ob.qm31_mul(a, b).tolist()
        assert list(V.q_inv(a)) == ob.qm31_inv(a).tolist()
        assert V.q_mul(a, V.q_inv(a)) == V.ONE
    for a in ((P - 1, P - 1, P - 1, P - 1), (1, 0, 0, 0), (0, 0, 0, 1), (0, 1, 0, 0)):
        assert list(V.q_inv(a)) == ob.qm31_inv(a).tolist()
    assert V.q_inv(V.ZERO) == V.ZERO                                # field.hpp: m_inv(0) = 0^(P-2) = 0


def _random_records(rnd, n_pi):
    rec = np.zeros((n_pi, 5), np.uint32)
    rec[:, 0] = rnd.integers(0, 1 << 32, n_pi, dtype=np.uint64)     # idx is any u32: taken mod P
    rec[:, 1:] = rnd.integers(0, P, (n_pi, 4))
    return rec


def test_sum_model_against_the_oracles_field_ops():
    """The per-term sum over random terms, every inverse and product taken by the oracle's QM31 functions."""
    rnd = np.random.default_rng(11)
    for n_pi in (0, 1, 3, 17):
        rec = _random_records(rnd, n_pi)
        z, alpha = (tuple(int(x) for x in rnd.integers(0, P, 4)) for _ in range(2))
        want = np.zeros(4, np.uint64)
        for r in rec:
            k = [int(r[0]) % P, 0, 0, 0]
            d = (np.array(r[1:5], np.uint64) + ob.qm31_mul(alpha, k) + P - np.array(z, np.uint64)) % P
            want = (want + ob.qm31_inv(d.astype(np.uint32))) % P
        got, bad = V.model(rec, z, alpha)
        assert got == want.tolist() and bad == 0


@pytest.mark.parametrize("n_pi", [1, 8, 9, 64, 65, 64 * 8, 64 * 8 + 1, 1000])
def test_batched_inversion_model_equals_the_per_term_model(n_pi):
    """Zeros at the first, a middle and the last position of a lane's chunk (lane 0: terms 0, 64, ..., 448), alone, two in
    one chunk, one in every lane, and a whole chunk of zeros: the batched form gives the per-term sum word for word."""
    rnd = np.random.default_rng(n_pi)
    z, alpha = (tuple(int(x) for x in rnd.integers(0, P, 4)) for _ in range(2))
    base = _random_records(rnd, n_pi)
    patterns = [[], [0], [n_pi - 1], [n_pi // 2], list(range(min(n_pi, 64)))]
    if n_pi > 64 * 7:
        patterns += [[0], [64 * 3], [64 * 7], [0, 64 * 7], [0, 64 * 3, 64 * 7], [64 * k for k in range(8)]]
    for zeros in patterns:
        rec = base.copy()
        for k in zeros:
            rec[k, 1:] = V.value_for_zero(rec[k, 0], z, alpha)
        dens, bad = V.denominators(rec, z, alpha)
        assert not bad and [k for k, d in enumerate(dens) if d == V.ZERO] == sorted(set(zeros))
        assert V.sum_batched(dens) == V.sum_per_term(dens), zeros


def test_noncanonical_words_count_as_zero_in_the_model():
    rnd = np.random.default_rng(3)
    z, alpha = (tuple(int(x) for x in rnd.integers(0, P, 4)) for _ in range(2))
    rec = _random_records(rnd, 5)
    for word in (P, 0xFFFFFFFF):
        bad_rec, zeroed = rec.copy(), rec.copy()
        bad_rec[2, 3], zeroed[2, 3] = word, 0
        got, bad = V.model(bad_rec, z, alpha)
        assert bad == 1 and (got, 0) == V.model(zeroed, z, alpha)


def test_many_input_circuit_is_a_sound_witness():
    """build_many: the oracle's two checks pass, the statement is variables 1 .. num_input, and two witnesses with different
    statements share one circuit."""
    a, b = V.build_many(17, first=11, seed=1), V.build_many(17, first=500, seed=2, bit=0)
    for w in (a, b):
        assert U.model_check(w.gates, w.witness_ops, w.variables) == U.NONE
        assert U.model_flow(w.gates, w.flow_wires, w.variables, w.unbound_flow())[0] == U.NONE
        assert [k for k, _ in w.inputs] == list(range(1, 18))
    assert np.array_equal(a.gates[:, [0, 1, 2, 4, 5]], b.gates[:, [0, 1, 2, 4, 5]]) and a.inputs[3:] != b.inputs[3:]
