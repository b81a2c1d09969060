"""Test helper (numpy, no device): the decommitment of a tree of the next proof, restated from stwo's conventions over
tests/commit_ref.py's layers.

- `node_layers`: every node of the mixed-size Merkle tree (commit_ref.merkle_root keeps only the root).
- `decommit(layers, queries, ob, b)`: stwo's batched decommitment (MerkleProver::decommit): layer by layer from the
  largest one down, the column values of the distinct queried nodes in ascending position, and for every distinct parent
  the child that is not itself queried; plus the cap (the nodes of layers 0 .. b in heap order, entry 0 zero) when b is
  given.
- `walk`: the other direction, the verifier's walk (oracle/rsv_oracle.c verify_trace_tree; SinglePathMerkleProof::
  from_stwo_proof): consumes the two lists in order, fails on a leftover, returns the root they hash to."""
import numpy as np

from tests import commit_ref as C

P = C.P


def node_layers(layers, ob):
    """layers {log: [n_cols, 2^log]} -> {l: uint32[2^l, 8]} for l = top .. 0."""
    top = max(layers)
    out, cur = {}, None
    for l in range(top, -1, -1):
        cols = layers.get(l)
        c = np.zeros((1 << l, 0), np.uint32) if cols is None else np.ascontiguousarray(np.asarray(cols, dtype=np.int64).T % P, dtype=np.uint32)
        if cur is None:
            cur = ob.hash_node(None, c)
        else:
            pairs = cur.reshape(-1, 2, 8)
            cur = ob.hash_node((np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])), c)
        out[l] = cur
    return out


def cap_of(nodes, b):
    """Heap order: layer l at entries 2^l .. 2^(l+1) - 1, entry 0 zero -> uint32[2^(b+1), 8]."""
    cap = np.zeros((2 << b, 8), np.uint32)
    for l in range(b + 1):
        cap[1 << l:2 << l] = nodes[l]
    return cap


def plan(queries, top):
    """The distinct queried nodes of every layer (ascending) and, per layer l >= 1, the witness positions."""
    pos = sorted({int(q) & ((1 << top) - 1) for q in queries})
    nodes, wit = {}, {}
    for l in range(top, -1, -1):
        cur = sorted({p >> (top - l) for p in pos})
        nodes[l] = cur
        have = set(cur)
        wit[l] = [x ^ 1 for x in cur if (x ^ 1) not in have] if l else []
    return nodes, wit


def decommit(layers, queries, ob, b=None, nodes=None):
    """-> (values uint32[nv], witness uint32[nw, 8], cap or None)."""
    top = max(layers)
    nodes = node_layers(layers, ob) if nodes is None else nodes
    at, wit = plan(queries, top)
    values, witness = [], []
    for l in range(top, -1, -1):
        if l in layers:
            cols = np.asarray(layers[l], dtype=np.int64)
            for x in at[l]:
                values.extend(int(v) % P for v in cols[:, x])
        witness.extend(nodes[l][x] for x in wit[l])
    w = np.array(witness, np.uint32).reshape(-1, 8)
    return np.array(values, np.uint32), w, None if b is None else cap_of(nodes, b)


def walk(values, witness, queries, ncols_at, top, ob):
    """verify_trace_tree's walk: the root the decommitment hashes to; AssertionError if a list runs out or is not used up."""
    values, witness = np.asarray(values, np.uint32), np.asarray(witness, np.uint32).reshape(-1, 8)
    pos = sorted({int(q) & ((1 << top) - 1) for q in queries})
    vi = hi = 0
    cur = {}
    nc = ncols_at.get(top, 0)
    for x in pos:
        assert vi + nc <= len(values)
        cur[x] = ob.hash_node(None, values[vi:vi + nc].reshape(1, nc))[0]
        vi += nc
    for layer in range(top - 1, -1, -1):
        nc = ncols_at.get(layer, 0)
        nxt = {}
        for x in sorted(cur):
            parent = x >> 1
            if parent in nxt:
                continue
            assert vi + nc <= len(values)
            c = values[vi:vi + nc].reshape(1, nc)
            vi += nc
            if (x ^ 1) in cur:
                sib = cur[x ^ 1]
            else:
                assert hi < len(witness)
                sib = witness[hi]
                hi += 1
            l, r = (sib, cur[x]) if x & 1 else (cur[x], sib)
            nxt[parent] = ob.hash_node((l.reshape(1, 8), r.reshape(1, 8)), c)[0]
        cur = nxt
    assert vi == len(values) and hi == len(witness), (vi, len(values), hi, len(witness))
    assert list(cur) == [0]
    return cur[0]
