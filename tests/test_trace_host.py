"""rsv_trace_log_sizes / rsv_trace_preprocessed (no device): the log sizes of the next proof's two components and their
50 preprocessed columns, host arithmetic over a shape's gate list and flow wires.  Pinned to the reference's fixture chain
(the header of fixture K+1 for every pair) and, column for column, to the oracle's restatement of pad() /
populate_logup_arguments / the Poseidon AIR's rows (oracle/recursion_circuit/trace.py) on circuits the oracle builds on the CPU."""
import ctypes

import numpy as np
import pytest

from tests.chain_harness import P, header_logs, oracle_circuit, pin_id, pins, round_constants


@pytest.mark.parametrize("pin", pins(), ids=pin_id)
def test_log_sizes_are_the_next_fixtures_header(rsv, pin):
    assert rsv.trace_log_sizes(pin["plonk_rows"], pin["poseidon_invocations"]) == header_logs(pin["dst"])


def test_log_sizes_edges(rsv):
    assert rsv.trace_log_sizes(1, 1) == (0, 8)            # 32 invocations minimum: 192 rows
    assert rsv.trace_log_sizes(4, 32) == (2, 8)
    assert rsv.trace_log_sizes(5, 33) == (3, 9)           # 48 invocations: 288 rows
    assert rsv.trace_log_sizes(1 << 20, 10912) == (20, 16)  # 10 912 * 6 = 65 472 <= 2^16
    assert rsv.trace_log_sizes((1 << 20) + 1, 10913) == (21, 17)  # padded to 10 928: 65 568 > 2^16
    for rows, flow in ((0, 5), (5, 0), ((1 << 24) + 1, 5), (5, 1 << 22)):
        with pytest.raises(rsv.RsvError) as e:
            rsv.trace_log_sizes(rows, flow)
        assert e.value.code == -2


def _call(rsv, gates, wires, lp, lq, plonk=None, poseidon=None):
    plonk = np.zeros((10, 1 << lp), np.uint32) if plonk is None else plonk
    poseidon = np.zeros((40, 1 << lq), np.uint32) if poseidon is None else poseidon
    u32p = ctypes.POINTER(ctypes.c_uint32)
    ptr = lambda a: a.ctypes.data_as(u32p) if a is not None else None
    rc = rsv.lib.rsv_trace_preprocessed(ptr(gates), 0 if gates is None else len(gates), ptr(wires), 0 if wires is None else len(wires), lp, lq,
                                        ptr(plonk), ptr(poseidon))
    return rc, plonk, poseidon


@pytest.mark.parametrize("src", ["small_proof.bin", "level10-1.bin"])
def test_preprocessed_columns_are_the_oracles(rsv, src):
    """The library's 10 + 40 columns from the UNPADDED gate list and flow wires == the oracle's pad() + plonk_columns /
    poseidon_columns preprocessed halves, bit for bit, at the next fixture's log sizes."""
    from oracle.recursion_circuit import trace as T
    pin = next(p for p in pins() if p["src"] == src)
    c, gates, wires = oracle_circuit(pin)
    lp, lq = header_logs(pin["dst"])
    assert rsv.trace_log_sizes(len(gates), len(wires)) == (lp, lq)
    rc_, plonk, poseidon = _call(rsv, gates, wires, lp, lq)
    assert rc_ == 0
    assert T.pad(c) == 1 << lp
    pre, _ = T.plonk_columns(c)
    for k, name in enumerate(T.PREPROCESSED):
        assert np.array_equal(plonk[k], np.asarray(pre[name], dtype=np.int64) % P), name
    qpre, _ = T.poseidon_columns(c.flow, round_constants(), lq, padding_hash=([0] * 8,))
    assert np.array_equal(poseidon, qpre.astype(np.int64)), [k for k in range(40) if not np.array_equal(poseidon[k], qpre[k].astype(np.int64))]
    # larger log sizes than needed: the same columns, zero-extended (the Poseidon rows behind the flow first and last)
    rc_, plonk2, poseidon2 = _call(rsv, gates, wires, lp + 1, lq + 1)
    assert rc_ == 0 and np.array_equal(plonk2[:, :1 << lp][[0, 1, 2, 7, 9]], plonk[[0, 1, 2, 7, 9]])
    assert (plonk2[3, 1 << lp:] == 1).all() and (plonk2[[0, 1, 2, 7, 8, 9], 1 << lp:] == 0).all()
    assert np.array_equal(poseidon2[:, :1 << lq], poseidon) and (poseidon2[:2, 1 << lq:] == 1).all() and (poseidon2[2:, 1 << lq:] == 0).all()


def test_argument_validation_writes_nothing(rsv):
    gates = np.array([[k, 0, k, 1, 0, 0] for k in range(4)] + [[1, 2, 4, 1, 0, 0], [4, 4, 5, 0, 5, 0]], np.uint32)
    wires = np.array([[1, 2, 5, 0, 3]], np.uint32)
    lp, lq = rsv.trace_log_sizes(len(gates), len(wires))
    rc_, plonk, poseidon = _call(rsv, gates, wires, lp, lq)
    assert rc_ == 0 and plonk[8, 5] == 1 and plonk[3].tolist() == [1, 1, 1, 1, 1, 0, 1, 1]

    def refused(code, gates, wires, lp, lq, null_plonk=False, null_poseidon=False):
        plonk = None if null_plonk else np.full((10, 1 << max(lp, 0)), 7, np.uint32)
        poseidon = None if null_poseidon else np.full((40, 1 << max(lq, 0)), 7, np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        ptr = lambda a: a.ctypes.data_as(u32p) if a is not None else None
        rc_ = rsv.lib.rsv_trace_preprocessed(ptr(gates), 0 if gates is None else len(gates), ptr(wires), 0 if wires is None else len(wires),
                                             lp, lq, ptr(plonk), ptr(poseidon))
        assert rc_ == code
        assert plonk is None or (plonk == 7).all()
        assert poseidon is None or (poseidon == 7).all()

    refused(-2, gates[:0], wires, lp, lq)                  # zero rows
    refused(-2, gates, wires[:0], lp, lq)                  # zero flow
    refused(-2, gates, wires, lp - 1, lq)                  # log sizes too small for the input
    refused(-2, gates, wires, lp, lq - 1)
    refused(-1, gates, wires, lp, lq, null_plonk=True)     # NULL outputs
    refused(-1, gates, wires, lp, lq, null_poseidon=True)
    refused(-1, None, wires, lp, lq)
    refused(-1, gates, None, lp, lq)
    bad = gates.copy()
    bad[2] = [2, 0, 2, 1, 0, 1]                            # not the constraint system's constant rows: num_input would differ
    refused(-5, bad, wires, lp, lq)
    twice = np.concatenate([gates, np.array([[5, 0, 6, 1, 0, 0]], np.uint32)])  # a Poseidon output used twice
    refused(-5, twice, wires, *rsv.trace_log_sizes(len(twice), 1))
    huge = wires.copy()
    huge[0, 0] = 1 << 30                                   # a wire beyond any program's variables
    refused(-5, gates, huge, lp, lq)
