"""The host side of the device serialiser, without a device: rsv_proof_bytes on the stored counts of every Poseidon fixture is
the file's length, the new entry points exist, and every refusal of rsv_proof_pack_dev comes before any device work."""
import ctypes

import pytest

from tests import oracle_binding as ob
from tests import pack_ref as PR
from tests.conftest import load_manifest, read_proof

POSEIDON = [e["file"] for e in load_manifest() if e["expect"] == "ok"]
E_NULL, E_SIZE = -1, -2


def test_there_are_15_fixtures():
    assert len(POSEIDON) == 15


@pytest.mark.parametrize("name", POSEIDON)
def test_length_of_the_stored_counts_is_the_file(rsv, name):
    proof = read_proof(name)
    lay = ob.proof_layout(proof)
    stored = {what: count for _, count, what in lay["prefixes"]}
    counts = [stored[f"queried_values[{t}]"] for t in range(4)] + [stored[f"hash_witness[{t}]"] for t in range(4)]
    for layer in ["first"] + [f"inner[{i}]" for i in range(lay["n_inner"])]:
        counts += [stored[layer + ".fri_witness"], stored[layer + ".hash_witness"]]
    assert rsv.proof_bytes_bound(lay["log_last"], 1 + lay["n_inner"], counts) == len(proof)
    assert counts == PR.counts_of(PR.fixture_parts(proof))


def test_length_by_hand_and_refusals(rsv):
    # T = 1, log_last = 0, nothing opened: the head, 2 + 4 * 4 + 2 + 4 * 2 words of empty decommitments, the nonce, the first
    # layer's 2 + 2 + 2 + 8, the u64(0) of the inner layers, the last layer's 2 + 4 + 1
    assert rsv.proof_bytes_bound(0, 1, [0] * 10) == 4 * (895 + 28 + 2 + 14 + 2 + 7)
    assert rsv.proof_bytes_bound(2, 3, [1, 2, 3, 4, 5, 6, 7, 8] + [9, 10] * 3) == 4 * (
        895 + 28 + 10 + 8 * 26 + 2 + 3 * 14 + 2 + 3 * (4 * 9 + 8 * 10) + 2 + 16 + 1)
    out = ctypes.c_size_t()
    counts = (ctypes.c_uint32 * 66)()
    assert rsv.lib.rsv_proof_bytes(0, 1, None, ctypes.byref(out)) == E_NULL and rsv.lib.rsv_proof_bytes(0, 1, counts, None) == E_NULL
    assert rsv.lib.rsv_proof_bytes(0, 0, counts, ctypes.byref(out)) == E_SIZE and rsv.lib.rsv_proof_bytes(0, 30, counts, ctypes.byref(out)) == E_SIZE
    assert rsv.lib.rsv_proof_bytes(17, 1, counts, ctypes.byref(out)) == E_SIZE and rsv.lib.rsv_proof_bytes(16, 29, counts, ctypes.byref(out)) == 0
    with pytest.raises(ValueError):
        rsv.proof_bytes_bound(0, 2, [0] * 10)


def test_entry_points_exist(rsv):
    for name in ("rsv_proof_bytes", "rsv_proof_pack_dev"):
        assert name in rsv.EXPORTS and hasattr(rsv.lib, name), name
    assert callable(rsv.proof_bytes_bound) and callable(rsv.Context.proof_pack) and callable(rsv.Chain.pack)
    assert rsv.lib.rsv_abi_version() == 6


def _parts(rsv, T=3, **change):
    """A ProofParts whose pointers are never dereferenced: every refusal comes first."""
    buf = 8192
    lists = {"values": [(buf, 16, buf, 1, 16)] * 4, "witness": [(buf, 128, buf, 1, 16)] * 4, "fri_witness": (buf, T * 64, buf, T, 16),
             "fri_hash_witness": (buf, T * 128, buf, T, 16)}
    words = {"log_size_plonk": 16, "log_size_poseidon": 15, "pow_bits": 20, "log_blowup": 1, "log_last": 0, "n_queries": 16, "n_layers": T}
    ptrs = {k: buf for k in ("d_sums", "d_roots", "d_root3", "d_samples", "d_samples3", "d_nonce", "d_fri_roots", "d_last_poly")}
    for k, v in change.items():
        if k in words:
            words[k] = v
        elif k in ptrs:
            ptrs[k] = v
        elif k in ("fri_witness", "fri_hash_witness"):
            lists[k] = v
        else:  # values2 = (...): one list of four
            lists[k[:-1]] = [v if t == int(k[-1]) else x for t, x in enumerate(lists[k[:-1]])]
    p = rsv.ProofParts(*words.values(), *ptrs.values())
    for t in range(4):
        p.values[t], p.witness[t] = rsv.ProofList(*lists["values"][t]), rsv.ProofList(*lists["witness"][t])
    p.fri_witness, p.fri_hash_witness = rsv.ProofList(*lists["fri_witness"]), rsv.ProofList(*lists["fri_hash_witness"])
    return p


def test_refusals_need_no_device(rsv):
    lib = rsv.lib
    fake = ctypes.create_string_buffer(64)  # never dereferenced: every refusal below comes first
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    buf, odd = 8192, 8194

    def call(parts=None, c=ctx, n=1, mask=None, blob=buf, cap=1 << 20, offsets=buf, **change):
        parts = _parts(rsv, **change) if parts is None else parts
        return lib.rsv_proof_pack_dev(c, ctypes.byref(parts), n, mask, blob, cap, offsets)

    assert call(c=None) == E_NULL and call(offsets=None) == E_NULL
    assert lib.rsv_proof_pack_dev(ctx, None, 1, None, buf, 1 << 20, buf) == E_NULL
    for k in ("d_sums", "d_roots", "d_root3", "d_samples", "d_samples3", "d_nonce", "d_fri_roots", "d_last_poly"):
        assert call(**{k: None}) == E_NULL, k
        assert call(**{k: odd}) == E_SIZE, k
    for t in range(4):
        assert call(**{f"values{t}": (None, 16, buf, 1, 16)}) == E_NULL and call(**{f"values{t}": (buf, 16, None, 1, 16)}) == E_NULL
        assert call(**{f"witness{t}": (None, 128, buf, 1, 16)}) == E_NULL and call(**{f"witness{t}": (buf, 128, None, 1, 16)}) == E_NULL
        assert call(**{f"values{t}": (odd, 16, buf, 1, 16)}) == E_SIZE and call(**{f"values{t}": (buf, 16, odd, 1, 16)}) == E_SIZE
        assert call(**{f"witness{t}": (odd, 128, buf, 1, 16)}) == E_SIZE and call(**{f"witness{t}": (buf, 128, odd, 1, 16)}) == E_SIZE
        assert call(**{f"values{t}": (buf, 15, buf, 1, 16)}) == E_SIZE and call(**{f"witness{t}": (buf, 127, buf, 1, 16)}) == E_SIZE  # stride < cap * width
    for k, width in (("fri_witness", 4), ("fri_hash_witness", 8)):
        assert call(**{k: (None, 3 * 16 * width, buf, 3, 16)}) == E_NULL and call(**{k: (buf, 3 * 16 * width, None, 3, 16)}) == E_NULL
        assert call(**{k: (odd, 3 * 16 * width, buf, 3, 16)}) == E_SIZE and call(**{k: (buf, 3 * 16 * width, odd, 3, 16)}) == E_SIZE
        assert call(**{k: (buf, 3 * 16 * width - 1, buf, 3, 16)}) == E_SIZE and call(**{k: (buf, 3 * 16 * width, buf, 2, 16)}) == E_SIZE
    assert call(n=0) == E_SIZE and call(n=(1 << 20) + 1) == E_SIZE
    assert call(n_queries=0) == E_SIZE and call(n_queries=129) == E_SIZE and call(log_blowup=0) == E_SIZE and call(log_blowup=17) == E_SIZE
    assert call(log_last=17) == E_SIZE and call(pow_bits=31) == E_SIZE
    assert call(n_layers=0) == E_SIZE and call(T=30) == E_SIZE
    assert call(blob=odd) == E_SIZE and call(offsets=8196) == E_SIZE and call(offsets=odd) == E_SIZE
    assert call(values0=(buf, 1 << 31, buf, 1, 1 << 31)) == E_SIZE  # one proof beyond 2^30 words


def test_chain_pack_needs_its_stages(rsv):
    ch = rsv.Chain.__new__(rsv.Chain)
    ch.done = {"open"}
    with pytest.raises(ValueError):
        ch.pack()
