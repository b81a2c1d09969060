"""tests/fri_open_ref.py and the host side of the FRI openings, without a device: the restated opening walks back to the roots
tests/fri_ref.py commits to, its counts are the stored counts of every Poseidon fixture (first layer and every inner layer,
at the fixture's own query positions), the new entry points exist, rsv_fri_open_sizes and its refusals, and the serialiser
(chain.proof_bytes) gives every fixture's bytes back from its own parts."""
import numpy as np
import pytest

from tests import commit_ref as C
from tests import fri_open_ref as FO
from tests import fri_ref as F
from tests import oracle_binding as ob
from tests.conftest import load_manifest, read_proof

P = C.P
POSEIDON = [e["file"] for e in load_manifest() if e["expect"] == "ok"]

# (sizes, log_last, b, queries or their number)
WALKS = {
    "three_sizes": ([8, 6, 5], 2, 1, 7),
    "A_is_M_minus_1": ([7, 6, 4], 1, 2, 5),
    "one_size_no_inner_layer": ([4], 2, 1, 3),
    "both_halves_of_a_pair_and_duplicates": ([7, 6, 5], 2, 1, [5, 4, 5, 100, 101, 37, 36 ^ 64, 127, 0, 0]),
    "one_query": ([6, 4], 1, 2, [33]),
}


@pytest.mark.parametrize("case", list(WALKS))
def test_walk_of_the_opening_gives_the_committed_roots(case):
    """Random columns through fri_ref.commit: for every tree the walk of open()'s two lists, with the queried values read off
    the columns, gives the root the commitment mixed; a list one entry short or long fails the walk."""
    sizes, log_last, b, queries = WALKS[case]
    rng = np.random.default_rng(2100 + list(WALKS).index(case))
    M = sizes[0]
    cols = {s: rng.integers(0, P, (4, 1 << s)) for s in sizes}
    if isinstance(queries, int):
        queries = rng.integers(0, 1 << M, queries).tolist()
    want = F.commit(cols, log_last, b, C.Channel(ob, np.zeros(8, np.uint32), 0), ob)
    assert len(want["roots"]) == 1 + F.n_inner_of(M, log_last, b)
    opened = FO.open_all(cols, want["layers"], queries, ob)
    for t, ((top, layers), (fw, hw, root)) in enumerate(zip(FO.trees(cols, want["layers"]), opened)):
        qs = [q >> (M - top) for q in queries]
        value = lambda l, x: layers[l][:, x]  # noqa: E731
        assert np.array_equal(root, want["roots"][t]), (case, t)
        assert np.array_equal(FO.walk(fw, hw, qs, value, top, set(layers), ob), want["roots"][t]), (case, t)
        for bad_f, bad_h in ((fw, hw[:-1]), (fw, np.concatenate([hw, hw[:1]]))) + (((fw[:-1], hw),) if len(fw) else ()):
            with pytest.raises(AssertionError):
                FO.walk(bad_f, bad_h, qs, value, top, set(layers), ob)


def test_every_position_queried_needs_no_witness():
    fri, hw = FO.plan(4, {4}, range(16))
    assert fri == [] and hw == []


@pytest.mark.parametrize("name", POSEIDON)
def test_counts_are_the_fixtures(name):
    """The stored fri_witness and hash_witness counts of the first layer and of every inner layer, from the fixture's own
    query positions."""
    proof = read_proof(name)
    lay = ob.proof_layout(proof)
    qM, M = C.query_positions(proof, ob)
    stored = {what: count for _, count, what in lay["prefixes"]}
    D = {M, lay["lp"] + lay["blowup"], lay["lq"] + lay["blowup"]}
    fri, hw = FO.plan(M, D, qM)
    assert (len(fri), len(hw)) == (stored["first.fri_witness"], stored["first.hash_witness"])
    assert lay["n_inner"] == M - 1 - lay["log_last"] - lay["blowup"]
    for i in range(lay["n_inner"]):
        top = M - 1 - i
        fri, hw = FO.plan(top, {top}, qM >> (M - top))
        assert (len(fri), len(hw)) == (stored[f"inner[{i}].fri_witness"], stored[f"inner[{i}].hash_witness"]), i
    nq = len(qM)
    assert stored["first.hash_witness"] <= nq * (M + 2 * (len(D) - 1))


def test_entry_points_exist(rsv):
    """The C-ABI exports, the 1:1 layer and the chain's stages."""
    for name in ("rsv_fri_open_sizes", "rsv_fri_open_dev"):
        assert name in rsv.EXPORTS and hasattr(rsv.lib, name), name
    assert callable(rsv.fri_open_sizes) and callable(rsv.Context.fri_open)
    assert callable(rsv.Chain.fri_open) and callable(rsv.Chain.proofs)
    assert rsv.lib.rsv_abi_version() == 6


def test_fri_open_sizes_and_refusals(rsv):
    assert rsv.fri_open_sizes([21, 20, 19], 1, 8, 80) == (240, 2000)
    assert rsv.fri_open_sizes([23, 21], 5, 8, 16) == (32, 16 * 25)
    assert rsv.fri_open_sizes([4], 1, 2, 128) == (128, 128 * 4)
    for bad in (([], 1, 1, 8), ([4, 4], 1, 1, 8), ([4, 5], 1, 1, 8), ([31], 1, 1, 8), ([4, 2], 1, 1, 8), ([4], 1, 3, 8), ([4], 0, 1, 8),
                ([30], 1, 17, 8), ([4], 1, 1, 0), ([4], 1, 1, 129), ([9] * 9, 1, 1, 8)):
        with pytest.raises(rsv.RsvError) as e:
            rsv.fri_open_sizes(*bad)
        assert e.value.code == -2, bad


@pytest.mark.parametrize("name", POSEIDON)
def test_serialiser_gives_the_fixture_back(rsv, name):
    """chain.proof_bytes on the parts of a fixture (oracle_binding.split_variable_part, the head's fields) is the file."""
    from importlib import import_module
    proof_bytes = import_module(rsv.__name__ + ".chain").proof_bytes
    proof = read_proof(name)
    w = np.frombuffer(proof, np.uint32)
    d = ob.split_variable_part(proof)
    lay = ob.proof_layout(proof)
    openings = [(np.array(d["queried_values"][t], np.uint32), np.array(d["hash_witness"][t], np.uint32).reshape(-1, 8)) for t in range(4)]
    layers = [(np.array(l["fri_witness"], np.uint32).reshape(-1, 4), np.array(l["hash_witness"], np.uint32).reshape(-1, 8), l["commitment"])
              for l in d["layers"]]
    got = proof_bytes(lay["lp"], lay["lq"], w[2:10].reshape(2, 4), (int(w[10]), lay["blowup"], lay["log_last"], lay["nq"]),
                      w[17:49].reshape(4, 8), ob.sampled_values(proof), openings, d["nonce"], layers, np.array(d["last"], np.uint32),
                      int(d["tail"][0]))
    assert len(d["tail"]) == 1 and got == proof
