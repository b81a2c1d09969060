"""rsv_proof_pack_dev / Chain.pack (`-m gpu`): the next proof serialised on the device.  Every comparison is exact on bytes
against chain.proof_bytes (pinned to the 15 fixtures by tests/test_fri_open_host.py) or against a fixture's file; blobs are
prefilled with 0xff so that an unwritten byte shows, and every buffer holds garbage past its count (tests/pack_ref.py)."""
from collections import defaultdict

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import pack_ref as PR
from tests.chain_harness import DEV, chain, inputs_of, mask_dev, masked_past_64, pin_of, program_of
from tests.conftest import fixture_cfg, load_manifest, read_proof

pytestmark = pytest.mark.gpu
POSEIDON = [e["file"] for e in load_manifest() if e["expect"] == "ok"]


@pytest.fixture(scope="module")
def ctx(rsv):
    c = rsv.Context(0)
    yield c
    c.close()


def _pack(rsv, ctx, hdr, plist, caps, mask=None, override=None, blob_bytes=None, blob_cap=None, with_blob=True):
    """-> (blob bytes as numpy uint8 (None without a blob), offsets as a list)."""
    import torch
    n = len(plist)
    parts, keep = PR.lay(rsv, hdr, plist, caps, override)
    if blob_bytes is None:
        blob_bytes = n * rsv.proof_bytes_bound(hdr[4], hdr[6], PR.caps_list(caps, hdr[6]))
    d_blob = torch.full((blob_bytes,), 0xFF, dtype=torch.uint8, device=DEV) if with_blob else None
    d_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
    ctx.proof_pack(parts, n, d_blob, d_offsets, d_mask=mask_dev(mask), blob_cap=blob_cap)
    ctx.synchronize()
    del keep
    return (d_blob.cpu().numpy() if with_blob else None), d_offsets.cpu().numpy().tolist()


def _check(blob, offsets, want):
    """want: per slot the bytes, b"" for an empty slot; the blob holds them back to back and the prefill behind."""
    assert offsets == np.cumsum([0] + [len(w) for w in want]).tolist()
    for k, w in enumerate(want):
        assert blob[offsets[k]:offsets[k + 1]].tobytes() == w, k
    assert (blob[offsets[-1]:] == 0xFF).all()


# ---------------------------------------------------------------- 1. the fixtures, without the chain
@pytest.mark.parametrize("name", POSEIDON)
def test_fixture_from_its_parts(rsv, ctx, name):
    proof = read_proof(name)
    hdr, p = PR.header_of(proof), PR.fixture_parts(proof)
    caps = PR.fixture_caps(rsv, hdr)
    assert all(c <= cap for c, cap in zip(PR.counts_of(p), PR.caps_list(caps, hdr[6])))
    blob, offsets = _pack(rsv, ctx, hdr, [p], caps)
    assert offsets == [0, len(proof)]
    _check(blob, offsets, [proof])


def _shapes():
    groups = defaultdict(list)
    for name in POSEIDON:
        groups[PR.header_of(read_proof(name))].append(name)
    return {"+".join(v): v for v in groups.values() if len(v) > 1}


SHARED = _shapes()


def test_some_fixtures_share_a_shape_and_differ_in_their_counts():
    differ = [names for names in SHARED.values() if len({tuple(PR.counts_of(PR.fixture_parts(read_proof(name)))) for name in names}) > 1]
    assert SHARED and differ


@pytest.mark.parametrize("names", list(SHARED.values()), ids=list(SHARED))
def test_fixtures_of_one_shape_as_a_batch(rsv, ctx, names):
    proofs = [read_proof(name) for name in names]
    hdr = PR.header_of(proofs[0])
    plist = [PR.fixture_parts(p) for p in proofs]
    blob, offsets = _pack(rsv, ctx, hdr, plist, PR.fixture_caps(rsv, hdr))
    _check(blob, offsets, proofs)


# ---------------------------------------------------------------- 2. random parts at the smallest shapes
CAPS = PR.CAPS


def _random_batch(rng, hdr, n):
    T, caps = hdr[6], PR.caps_list(CAPS, hdr[6])
    plist = []
    for _ in range(n):
        counts = [int(rng.choice([0, 1, cap - 1, cap])) for cap in caps]
        plist.append(PR.random_parts(rng, T, hdr[4], counts))
    return plist


@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("log_last", [0, 2])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_random_parts(rsv, ctx, T, log_last, n):
    rng = np.random.default_rng(2500 + 100 * T + 10 * log_last + n)
    hdr = (7, 6, 3, 1, log_last, 2, T)
    plist = _random_batch(rng, hdr, n)
    mask = masked_past_64(n) if n == 70 else None
    over = {}
    if n > 1:  # one count of proof 1 is cap + 1: its slot is empty, its neighbours unchanged
        i = int(rng.integers(0, 8 + 2 * T))
        over[(1, i)] = PR.caps_list(CAPS, T)[i] + 1
    want = [b"" if (mask and not mask[k]) or (k == 1 and over) else PR.expected(rsv, hdr, p) for k, p in enumerate(plist)]
    assert all(len(w) == rsv.proof_bytes_bound(log_last, T, PR.counts_of(p)) for w, p in zip(want, plist) if w)
    blob, offsets = _pack(rsv, ctx, hdr, plist, CAPS, mask=mask, override=over)
    _check(blob, offsets, want)


def test_offsets_past_one_step_of_the_scan(rsv, ctx):
    """1 030 proofs: the scan's second step of 1 024 starts from the carry of the first."""
    rng = np.random.default_rng(2599)
    hdr = (7, 6, 3, 1, 0, 2, 1)
    distinct = _random_batch(rng, hdr, 5)
    plist = [distinct[k % 5] for k in range(1030)]
    each = [PR.expected(rsv, hdr, p) for p in distinct]
    blob, offsets = _pack(rsv, ctx, hdr, plist, CAPS)
    _check(blob, offsets, [each[k % 5] for k in range(1030)])


# ---------------------------------------------------------------- 3. offsets only, and a blob that is too small
def test_offsets_only_and_a_blob_too_small(rsv, ctx):
    rng = np.random.default_rng(2600)
    hdr = (7, 6, 3, 1, 2, 2, 2)
    plist = _random_batch(rng, hdr, 5)
    want = [PR.expected(rsv, hdr, p) for p in plist]
    blob, offsets = _pack(rsv, ctx, hdr, plist, CAPS)
    _check(blob, offsets, want)
    none, only = _pack(rsv, ctx, hdr, plist, CAPS, with_blob=False)
    assert none is None and only == offsets
    exact, again = _pack(rsv, ctx, hdr, plist, CAPS, blob_bytes=offsets[5])
    assert again == offsets and exact.tobytes() == b"".join(want)
    k = 2  # the blob ends where proof 2 begins: proofs 0 and 1 are written, nothing from there on
    short, again = _pack(rsv, ctx, hdr, plist, CAPS, blob_cap=offsets[k])
    assert again == offsets and again[5] > offsets[k]
    assert short[:offsets[k]].tobytes() == b"".join(want[:k]) and (short[offsets[k]:] == 0xFF).all()
    # a capacity inside proof 1: proof 0 alone
    short, again = _pack(rsv, ctx, hdr, plist, CAPS, blob_cap=offsets[2] - 4)
    assert again == offsets and short[:offsets[1]].tobytes() == want[0] and (short[offsets[1]:] == 0xFF).all()


# ---------------------------------------------------------------- 4. the loop closes on the device
def _whole(rsv, ctx, wp, batch, inputs, cfg):
    ch = chain(rsv, ctx, wp, batch, inputs, cfg.log_blowup_factor, upto="fri", caps=True, log_last=cfg.log_last_layer_degree_bound)
    with pytest.raises(ValueError):
        ch.pack()  # needs open() and fri_open() first
    ch.pow(cfg.pow_bits, cfg.n_queries)
    ch.open()
    ch.fri_open()
    return ch


def _verify(rsv, ctx, d_blob, d_offsets, n, name):
    import torch
    acc = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    reason = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    ctx.verify_batch(d_blob, d_offsets, n, acc, reason, cfg=fixture_cfg(name), inputs=inputs_of(name))
    ctx.synchronize()
    return acc.cpu().tolist(), reason.cpu().tolist()


def test_two_levels_without_leaving_the_device(rsv, ctx):
    pin1, pin2 = pin_of("level1-5.bin"), pin_of("level2-1.bin")
    assert (pin1["dst"], pin2["dst"]) == ("level2-1.bin", "level3-1.bin")
    want2, want3 = read_proof("level2-1.bin"), read_proof("level3-1.bin")
    wp1 = program_of(rsv, pin1)
    ch1 = _whole(rsv, ctx, wp1, [read_proof("level1-5.bin")], inputs_of("level1-5.bin"), fixture_cfg("level2-1.bin"))
    d_blob, d_offsets = ch1.pack()
    assert d_blob.is_cuda and d_offsets.is_cuda
    assert _verify(rsv, ctx, d_blob, d_offsets, 1, "level2-1.bin") == ([1], [0])
    # the same pair into the next level's chain: nothing has been copied to the host up to here
    wp2 = program_of(rsv, pin2)
    cfg3 = fixture_cfg("level3-1.bin")
    ch2 = rsv.Chain(ctx, wp2, 1, cfg3.log_blowup_factor, log_last=cfg3.log_last_layer_degree_bound, fill=0xFFFFFFFF, caps=True, device=DEV)
    ch2.witness((d_blob, d_offsets), inputs_of("level2-1.bin"))
    for stage in ("trace", "commit", "tree3", "sample", "fri"):
        getattr(ch2, stage)()
    ch2.pow(cfg3.pow_bits, cfg3.n_queries)
    ch2.open()
    ch2.fri_open()
    blob3, offsets3 = ch2.pack(exact=True)
    assert offsets3.cpu().tolist() == [0, len(want3)] and blob3.numel() == len(want3)
    assert blob3.cpu().numpy().tobytes() == want3
    # and level 1's blob against the host path and the file
    offsets = d_offsets.cpu().tolist()
    blob = d_blob.cpu().numpy()
    assert offsets == [0, len(want2)]
    assert blob[:len(want2)].tobytes() == want2 == ch1.proofs()[0]
    assert (blob[len(want2):] == 0xFF).all()
    wp1.close()
    wp2.close()


def test_batch_with_a_tampered_middle_proof(rsv, ctx):
    pin = pin_of("level1-5.bin")
    proof, want = read_proof("level1-5.bin"), read_proof("level2-1.bin")
    wp = program_of(rsv, pin)
    ch = _whole(rsv, ctx, wp, [proof, ob.tamper(proof, 5), proof], inputs_of("level1-5.bin"), fixture_cfg("level2-1.bin"))
    d_blob, d_offsets = ch.pack()
    acc, reason = _verify(rsv, ctx, d_blob, d_offsets, 3, "level2-1.bin")
    offsets, blob = d_offsets.cpu().tolist(), d_blob.cpu().numpy()
    assert offsets == [0, len(want), len(want), 2 * len(want)]
    _check(blob, offsets, [want, b"", want])
    assert acc == [1, 0, 1] and reason == [0, 1, 0]  # an empty proof does not parse (tests/test_gpu_parity.py, truncations)
    exact, offsets_exact = ch.pack(exact=True)
    assert offsets_exact.cpu().tolist() == offsets and exact.cpu().numpy().tobytes() == want + want
    wp.close()
