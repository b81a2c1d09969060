"""The configuration grid's table (tests/verify_grid.py), checked without a device: every point is a configuration the
library admits on its shape, the boundary values the grid exists for are in it by name, and the library's host arithmetic
(rsv_fri_sizes) agrees with the oracle's rule at every point."""
import pytest

from tests import verify_grid as G


@pytest.fixture(scope="module")
def logs():
    return {shape: G.logs_of(shape) for shape in G.SHAPES}


def test_shapes_are_the_ones_the_grid_was_laid_out_for(logs):
    assert logs == {"S1": (6, 8), "S2": (12, 8), "S3": (7, 9), "R": (16, 15), "R17": (17, 16)}


def test_points_are_distinct_and_few_enough_to_run(rsv):
    assert len(set(G.POINTS)) == len(G.POINTS)
    assert all(p[0] in G.SHAPES for p in G.POINTS)
    # a verify call carries at most 16 configurations: R's points fit one call, the S points two
    assert len([p for p in G.POINTS if p[0] in G.R_SRCS]) <= rsv.MAX_CFGS < len([p for p in G.POINTS if p[0] not in G.R_SRCS]) <= 2 * rsv.MAX_CFGS


@pytest.mark.parametrize("point", G.POINTS, ids=G.point_id)
def test_every_point_is_admitted_and_sized_by_the_oracles_rule(rsv, logs, point):
    lp, lq = logs[point[0]]
    _shape, pow_bits, b, ll, nq = point
    assert rsv.cfg_check(rsv.PcsConfig(pow_bits, b, ll, nq))
    got = rsv.fri_sizes(lp, lq, b, ll)
    M, A, B, n_inner = G.sizes_of(lp, lq, point)
    assert (M, A, B) == (max(lp + 1, lq + 2) + b, lp + b, lq + b) and n_inner == M - 1 - ll - b
    assert got["sizes"] == sorted({M, A, B}, reverse=True) and len(got["sizes"]) == 3
    assert got["n_inner"] == n_inner >= 1


def test_a_point_outside_the_limits_is_refused(rsv, logs):
    """What makes the test above say something: cfg_check and fri_sizes do refuse."""
    assert not rsv.cfg_check(rsv.PcsConfig(2, 1, 0, 129)) and not rsv.cfg_check(rsv.PcsConfig(2, 1, 0, 0))
    assert not rsv.cfg_check(rsv.PcsConfig(2, 17, 0, 9)) and not rsv.cfg_check(rsv.PcsConfig(2, 1, 17, 9))
    with pytest.raises(rsv.RsvError) as e:
        rsv.fri_sizes(*logs["R"], 1, 15)                    # a column no larger than the last layer
    assert e.value.code == -2


def test_every_point_has_an_accepting_proof(logs):
    """log_last = min(lp, lq) - 1 is a configuration rsv_fri_sizes answers and no proof verifies under: the smallest column
    would meet no inner layer (the chain made proofs there that both verifiers rejected with RSV_R_FRI_LAST, and
    rsv_witness_fri_dev refuses it since: tests/test_verify_grid_gpu.py).  Three points the grid was first laid out with
    were of that kind; each shape's largest log_last is in the table instead, and 14 on the smallest shape that takes it."""
    assert all(G.provable(*logs[p[0]], p) for p in G.POINTS)
    for gone in (("S2", 2, 2, 7, 6), ("R", 2, 1, 14, 16), ("S1", 2, 1, 5, 12)):
        assert not G.provable(*logs[gone[0]], gone) and gone not in G.POINTS
        kept = gone[:3] + (gone[3] - 1,) + gone[4:]
        assert G.provable(*logs[kept[0]], kept) and kept in G.POINTS
    assert ("R17", 2, 1, 14, 16) in G.POINTS and not G.provable(*logs["R17"], ("R17", 2, 1, 15, 16))


def test_boundary_values_are_in_the_table_by_name():
    """A later trim of the table cannot drop these silently."""
    def has(shape=None, pow_bits=None, b=None, ll=None, nq=None):
        want = (shape, pow_bits, b, ll, nq)
        return any(all(w is None or w == v for w, v in zip(want, p)) for p in G.POINTS)

    for nq in (1, 4, 32, 33, 64, 65, 128):
        assert has(shape="S1", nq=nq) and has(shape="R", nq=nq), nq
    assert has(shape="S1", nq=3)
    for ll in (3, 4, 5, 9, 14):
        assert has(ll=ll), ll
    assert has(pow_bits=0) and has(b=16)
    # the Q axis in full on the small domain, and both domains at the largest count
    assert all(has(shape="S1", b=1, ll=0, nq=nq) for nq in G.Q_SMALL)
    assert has(shape="S1", b=1, nq=128) and has(shape="R", b=1, nq=128)


def test_the_two_domains_of_the_query_axis(logs):
    """128 queries saturate S1's Plonk domain (2^7 positions) and stay sparse on R's (2^17)."""
    lp, lq = logs["S1"]
    assert G.sizes_of(lp, lq, ("S1", 2, 1, 0, 128))[1] == 7
    lp, lq = logs["R"]
    M, A, B, n_inner = G.sizes_of(lp, lq, ("R", 2, 1, 8, 128))
    assert (M, A, B, n_inner) == (18, 17, 16, 8)
    assert G.sizes_of(*logs["R"], ("R", 2, 1, 13, 16))[3] == 3 and G.sizes_of(*logs["R17"], ("R17", 2, 1, 14, 16))[3] == 3
