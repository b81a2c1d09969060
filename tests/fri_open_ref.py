"""Test helper (numpy, no device): the opening of a FRI layer tree of the next proof, stwo's pair-tree decommitment restated
over tests/decommit_ref.py's node layers.

A tree has leaves at `top` and a QM31 value (four M31 words) per node at its data layers D: the first layer's tree at every
quotient column's log size, an inner layer's tree at `top` alone.  With Q_l the distinct (query >> (top - l)) ascending,
S_l = Q_l and their siblings (x ^ 1) at a data layer, Q_l elsewhere; Q_(l-1) derives from Q_l, not from S_l.

- `sets`, `plan`: Q and S, and the positions both lists name: fri_witness, for l in D descending, the x in S_l ascending
  that no query reaches; hash_witness, for l = top - 1 .. 0 and x in S_l ascending, the children 2x, 2x + 1 that are not in
  S_(l+1), left first (a sibling-only node of a lower data layer gives both).
- `open`: the two lists from the columns and the node layers.
- `walk`: the consumer's direction (SinglePairMerkleProof::from_stwo_proof): rebuilds the nodes of every S_l from the
  values (the queried ones given, the others taken from fri_witness) and the hash witness, fails on a list that runs out
  or is not used up, returns the root."""
import numpy as np

from tests import commit_ref as C

P = C.P


def sets(top, D, queries):
    """-> (Q, S): {l: ascending list} for l = top .. 0; queries at `top` bits (higher bits ignored)."""
    pos = sorted({int(q) & ((1 << top) - 1) for q in queries})
    Q, S = {}, {}
    for l in range(top, -1, -1):
        Q[l] = sorted({p >> (top - l) for p in pos})
        S[l] = sorted(set(Q[l]) | {x ^ 1 for x in Q[l]}) if l in D else Q[l]
    return Q, S


def plan(top, D, queries):
    """-> ([(l, x)] of fri_witness, [(l, x)] of hash_witness (l the node's own layer)), in list order."""
    Q, S = sets(top, set(D), queries)
    fri = [(l, x) for l in sorted(D, reverse=True) for x in S[l] if x not in set(Q[l])]
    hw = []
    for l in range(top - 1, -1, -1):
        have = set(S[l + 1])
        hw += [(l + 1, c) for x in S[l] for c in (2 * x, 2 * x + 1) if c not in have]
    return fri, hw


def open(layers, top, queries, nodes):  # noqa: A001
    """layers {l: QM31 column (4, 2^l)} (the data layers), nodes decommit_ref.node_layers of them -> (fri_witness
    uint32[nf, 4], hash_witness uint32[nh, 8])."""
    assert max(layers) == top
    fri, hw = plan(top, set(layers), queries)
    fw = np.array([[int(v) % P for v in np.asarray(layers[l])[:, x]] for l, x in fri], np.uint32).reshape(-1, 4)
    return fw, np.array([nodes[l][x] for l, x in hw], np.uint32).reshape(-1, 8)


def walk(fri_witness, hash_witness, queries, queried, top, D, ob):
    """queried(l, x) -> the four words of the value a query reaches (x in Q_l, l in D).  -> the root; AssertionError if a
    list runs out or is not used up."""
    fri_witness = np.asarray(fri_witness, np.uint32).reshape(-1, 4)
    hash_witness = np.asarray(hash_witness, np.uint32).reshape(-1, 8)
    D = set(D)
    Q, S = sets(top, D, queries)
    fi = hi = 0
    prev = None
    for l in range(top, -1, -1):
        cur = {}
        for x in S[l]:
            if l in D:
                if x in set(Q[l]):
                    v = np.array([int(w) % P for w in queried(l, x)], np.uint32)
                else:
                    assert fi < len(fri_witness), "fri_witness ran out"
                    v = fri_witness[fi]
                    fi += 1
                cols = v.reshape(1, 4)
            else:
                assert l != top
                cols = np.zeros((1, 0), np.uint32)
            if l == top:
                cur[x] = ob.hash_node(None, cols)[0]
                continue
            kids = []
            for c in (2 * x, 2 * x + 1):
                if c not in prev:
                    assert hi < len(hash_witness), "hash_witness ran out"
                    prev[c] = hash_witness[hi]
                    hi += 1
                kids.append(np.ascontiguousarray(prev[c]).reshape(1, 8))
            cur[x] = ob.hash_node((kids[0], kids[1]), cols)[0]
        prev = cur
    assert fi == len(fri_witness) and hi == len(hash_witness), (fi, len(fri_witness), hi, len(hash_witness))
    assert list(prev) == [0]
    return prev[0]


def trees(cols, inner):
    """cols {size: (4, 2^size)} (the quotient columns), inner the inner layers' evaluations (fri_ref.commit's "layers") ->
    [(top, data layers)] per tree: the first layer, then inner layer i at top = M - 1 - i."""
    M = max(cols)
    return [(M, dict(cols))] + [(M - 1 - i, {M - 1 - i: ev}) for i, ev in enumerate(inner)]


def open_all(cols, inner, queries, ob, node_cache=None):
    """-> per tree (fri_witness, hash_witness, root) at queries of M bits; node_cache (a list) keeps the node layers."""
    from tests import decommit_ref as D
    M = max(cols)
    out = []
    for top, layers in trees(cols, inner):
        nodes = D.node_layers({l: np.asarray(c, dtype=np.int64) for l, c in layers.items()}, ob)
        if node_cache is not None:
            node_cache.append(nodes)
        fw, hw = open(layers, top, [(int(q) & ((1 << M) - 1)) >> (M - top) for q in queries], nodes)
        out.append((fw, hw, nodes[0][0]))
    return out
