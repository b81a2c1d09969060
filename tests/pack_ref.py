"""What the serialiser's test modules share (no test lives here): the parts of a proof as arrays (a fixture's, or random ones),
the bytes chain.proof_bytes gives for them, their counts in rsv_proof_bytes' order, and lay(), which puts a batch of parts
into capacity-padded device buffers with garbage past every count and points an rsv.ProofParts at them.
Nothing here needs a device to import; torch is imported where a helper touches one."""
from importlib import import_module

import numpy as np

from tests import oracle_binding as ob

GARBAGE = 0xDEADBEEF
CAPS = ([3, 5, 4, 6], [4, 3, 5, 2], 3, 4)  # the capacities of the random parts' buffers, in caps_list's form


def header_of(proof):
    """(lp, lq, pow_bits, log_blowup, log_last, n_queries, T) of a fixture."""
    lay = ob.proof_layout(proof)
    w = np.frombuffer(proof, np.uint32)
    return (lay["lp"], lay["lq"], int(w[10]), lay["blowup"], lay["log_last"], lay["nq"], 1 + lay["n_inner"])


def fixture_parts(proof):
    """The parts of a fixture: the head's fields and oracle_binding.split_variable_part."""
    w = np.frombuffer(proof, np.uint32)
    d = ob.split_variable_part(proof)
    assert len(d["tail"]) == 1
    samples = ob.sampled_values(proof)
    return {"sums": w[2:10].copy(), "roots": w[17:41].copy(), "root3": w[41:49].copy(), "samples": samples[:134].reshape(-1),
            "samples3": samples[134:].reshape(-1), "nonce": np.array(d["nonce"], np.uint32),
            "fri_roots": np.concatenate([l["commitment"] for l in d["layers"]]),
            "last_poly": np.array(d["last"], np.uint32).reshape(-1),
            "values": [np.array(d["queried_values"][t], np.uint32).reshape(-1) for t in range(4)],
            "witness": [np.array(d["hash_witness"][t], np.uint32).reshape(-1, 8) for t in range(4)],
            "fri_witness": [np.array(l["fri_witness"], np.uint32).reshape(-1, 4) for l in d["layers"]],
            "fri_hash_witness": [np.array(l["hash_witness"], np.uint32).reshape(-1, 8) for l in d["layers"]]}


def random_parts(rng, T, log_last, counts):
    """Random words in every part; counts in rsv_proof_bytes' order."""
    r = lambda *shape: rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    return {"sums": r(8), "roots": r(24), "root3": r(8), "samples": r(536), "samples3": r(32), "nonce": r(2), "fri_roots": r(8 * T),
            "last_poly": r(4 << log_last), "values": [r(counts[t]) for t in range(4)], "witness": [r(counts[4 + t], 8) for t in range(4)],
            "fri_witness": [r(counts[8 + 2 * t], 4) for t in range(T)], "fri_hash_witness": [r(counts[9 + 2 * t], 8) for t in range(T)]}


def counts_of(p):
    out = [len(v) for v in p["values"]] + [len(w) for w in p["witness"]]
    for f, h in zip(p["fri_witness"], p["fri_hash_witness"]):
        out += [len(f), len(h)]
    return out


def expected(rsv, hdr, p):
    """chain.proof_bytes on the parts: the definition of the bytes."""
    proof_bytes = import_module(rsv.__name__ + ".chain").proof_bytes
    lp, lq, pow_bits, b, last, nq, T = hdr
    layers = [(p["fri_witness"][t], p["fri_hash_witness"][t], p["fri_roots"][8 * t:8 * t + 8]) for t in range(T)]
    return proof_bytes(lp, lq, p["sums"], (pow_bits, b, last, nq), np.concatenate([p["roots"], p["root3"]]).reshape(4, 8),
                       np.concatenate([p["samples"], p["samples3"]]).reshape(142, 4), list(zip(p["values"], p["witness"])), p["nonce"], layers,
                       p["last_poly"], last)


def caps_list(caps, T):
    """caps = (values caps [4], witness caps [4], fri_witness cap, fri_hash_witness cap) in rsv_proof_bytes' order."""
    vcaps, wcaps, fv, fw = caps
    return list(vcaps) + list(wcaps) + [fv, fw] * T


def lay(rsv, hdr, plist, caps, count_override=None, device="cuda:0"):
    """The parts of a batch in device buffers as the chain leaves them: the values of trees 0-2 in one buffer at their
    trees' offsets with counts [n, 3], the witness nodes of trees 0-2 in [n, 3, cap, 8] (cap: the largest of the three), tree
    3 apart, the layer trees in [n, T, cap, width] with counts [n, T]; every word past a count is GARBAGE.
    count_override {(proof, index in rsv_proof_bytes' order): count} stores another count than the items laid.
    -> (rsv.ProofParts, the tensors it points into)."""
    import torch
    vcaps, wcaps, fv, fw = caps
    n, T, last = len(plist), hdr[6], hdr[4]
    vat = np.cumsum([0] + list(vcaps[:3]))
    wcap = max(wcaps[:3])
    g = lambda *shape: np.full(shape, GARBAGE, np.uint32)  # noqa: E731
    a = {"sums": g(n, 8), "roots": g(n, 24), "root3": g(n, 8), "samples": g(n, 536), "samples3": g(n, 32), "nonce": g(n, 2),
         "fri_roots": g(n, 8 * T), "last_poly": g(n, 4 << last), "values": g(n, int(vat[3])), "n_values": g(n, 3), "witness": g(n, 3, wcap, 8),
         "n_witness": g(n, 3), "values3": g(n, vcaps[3]), "n_values3": g(n), "witness3": g(n, wcaps[3], 8), "n_witness3": g(n),
         "fri_witness": g(n, T, fv, 4), "n_fri_witness": g(n, T), "fri_hash_witness": g(n, T, fw, 8), "n_fri_hash_witness": g(n, T)}
    for k, p in enumerate(plist):
        for key in ("sums", "roots", "root3", "samples", "samples3", "nonce", "fri_roots", "last_poly"):
            a[key][k] = p[key]
        c = counts_of(p)
        for t in range(3):
            a["values"][k, vat[t]:vat[t] + c[t]] = p["values"][t]
            a["witness"][k, t, :c[4 + t]] = p["witness"][t]
            a["n_values"][k, t], a["n_witness"][k, t] = c[t], c[4 + t]
        a["values3"][k, :c[3]], a["witness3"][k, :c[7]] = p["values"][3], p["witness"][3]
        a["n_values3"][k], a["n_witness3"][k] = c[3], c[7]
        for t in range(T):
            a["fri_witness"][k, t, :c[8 + 2 * t]], a["fri_hash_witness"][k, t, :c[9 + 2 * t]] = p["fri_witness"][t], p["fri_hash_witness"][t]
            a["n_fri_witness"][k, t], a["n_fri_hash_witness"][k, t] = c[8 + 2 * t], c[9 + 2 * t]
    for (k, i), v in (count_override or {}).items():
        if i < 3:
            a["n_values"][k, i] = v
        elif i == 3:
            a["n_values3"][k] = v
        elif i < 7:
            a["n_witness"][k, i - 4] = v
        elif i == 7:
            a["n_witness3"][k] = v
        else:
            a["n_fri_hash_witness" if i & 1 else "n_fri_witness"][k, (i - 8) >> 1] = v
    d = {key: torch.from_numpy(v.view(np.int32)).to(device) for key, v in a.items()}
    parts = rsv.ProofParts(*hdr, *(d[key].data_ptr() for key in ("sums", "roots", "root3", "samples", "samples3", "nonce", "fri_roots", "last_poly")))
    for t in range(3):
        parts.values[t] = rsv.proof_list(d["values"], int(vat[3]), d["n_values"], 3, vcaps[t], items_at=int(vat[t]), count_at=t)
        parts.witness[t] = rsv.proof_list(d["witness"], 3 * wcap * 8, d["n_witness"], 3, wcaps[t], items_at=t * wcap * 8, count_at=t)
    parts.values[3] = rsv.proof_list(d["values3"], vcaps[3], d["n_values3"], 1, vcaps[3])
    parts.witness[3] = rsv.proof_list(d["witness3"], wcaps[3] * 8, d["n_witness3"], 1, wcaps[3])
    parts.fri_witness = rsv.proof_list(d["fri_witness"], T * fv * 4, d["n_fri_witness"], T, fv)
    parts.fri_hash_witness = rsv.proof_list(d["fri_hash_witness"], T * fw * 8, d["n_fri_hash_witness"], T, fw)
    return parts, d


def fixture_caps(rsv, hdr):
    """The capacities the chain's buffers have for a fixture's shape: decommit_sizes of trees 0-3, fri_open_sizes."""
    lp, lq, _, b, last, nq, _ = hdr
    trees = [rsv.decommit_sizes([(lp, x), (lq, y)], b, nq) for x, y in ((10, 40), (12, 48), (8, 8))]
    trees.append(rsv.decommit_sizes([(rsv.composition_log_size(lp, lq), 8)], b, nq))
    fv, fw = rsv.fri_open_sizes(rsv.fri_sizes(lp, lq, b, last)["sizes"], b, last, nq)
    return [v for v, _ in trees], [w for _, w in trees], fv, fw
