"""Test helper (numpy, no device): proof of work and queries of the next proof, restated from the verifier's transcript
(oracle/rsv_oracle.c run_transcript): the nonce is mixed as the QM31 (nonce & (2^22 - 1), (nonce >> 22) & (2^21 - 1),
(nonce >> 43) & (2^21 - 1), 0), it qualifies when word 0 of the digest behind that mix has pow_bits low zero bits, and the
queries are the words of the ceil(n_queries / 8) draws that follow, each cut to its low bits.  The permutation is the
oracle's (poseidon2_permute over batches of candidates); the channel is commit_ref.Channel."""
import numpy as np

from tests import commit_ref as C
from tests import fri_ref as F

BATCH = 1 << 16


def nonce_words(nonce):
    nonce = np.asarray(nonce, dtype=np.uint64)
    return (nonce & np.uint64((1 << 22) - 1), (nonce >> np.uint64(22)) & np.uint64((1 << 21) - 1), (nonce >> np.uint64(43)) & np.uint64((1 << 21) - 1))


def qualifying(digest, pow_bits, nonces, ob):
    """bool per nonce (uint64 array): the digest behind the mix of the nonce has pow_bits low zero bits in word 0."""
    nonces = np.asarray(nonces, dtype=np.uint64)
    st = np.zeros((len(nonces), 16), np.uint32)
    for k, w in enumerate(nonce_words(nonces)):
        st[:, k] = w.astype(np.uint32)
    st[:, 8:] = np.asarray(digest, np.uint32)
    return (ob.poseidon2_permute(st)[:, 8] & np.uint32((1 << pow_bits) - 1)) == 0


def grind(channel, pow_bits, start, max_tries, ob):
    """The smallest qualifying nonce in [start, start + max_tries), or None; channel: its first eight words are the digest."""
    digest = np.asarray(channel, np.uint32)[:8]
    for at in range(start, start + max_tries, BATCH):
        n = min(BATCH, start + max_tries - at)
        nonces = np.uint64(at) + np.arange(n, dtype=np.uint64)
        hit = np.flatnonzero(qualifying(digest, pow_bits, nonces, ob))
        if len(hit):
            return at + int(hit[0])
    return None


def mix_nonce(channel, nonce, ob):
    """channel uint32[16] (digest, n_sent, zeros) -> the channel behind the mix of the nonce, same form."""
    ch = C.Channel(ob, np.asarray(channel, np.uint32)[:8])
    ch.mix_one([int(w) for w in nonce_words(nonce)] + [0])
    out = np.zeros(16, np.uint32)
    out[:8] = ch.digest
    return out


def draw_queries(channel, n_queries, log_size, log_size_low, ob):
    """channel uint32[16] -> (queries uint32[n_queries] of log_size bits in draw order, the same >> (log_size -
    log_size_low), the channel behind the draws)."""
    channel = np.asarray(channel, np.uint32)
    ch = C.Channel(ob, channel[:8], int(channel[8]))
    words = []
    for _ in range((n_queries + 7) // 8):
        lo, hi = ch.draw()
        words += list(lo) + list(hi)
    q = np.array(words[:n_queries], dtype=np.uint32) & np.uint32((1 << log_size) - 1)
    out = channel.copy()
    out[8] = ch.n_sent
    return q, q >> np.uint32(log_size - log_size_low), out


def channel_before_pow(proof, ob):
    """The channel of a proof's own transcript in front of its proof of work, rebuilt from the proof's values (roots, claimed
    sums, sampled values, FRI roots, last polynomial): uint32[16] (digest, n_sent = 0, zeros)."""
    lay = ob.proof_layout(proof)
    w = np.frombuffer(proof, dtype=np.uint32)
    roots = [w[17 + 8 * t:25 + 8 * t] for t in range(4)]
    sums = (tuple(int(v) for v in w[2:6]), tuple(int(v) for v in w[6:10]))
    _, _, _, ch = C.transcript_prefix(roots[:3], lay["lp"], lay["lq"], sums, ob)
    ch.mix(roots[3])
    ch.draw()
    F.begin(ch, ob.sampled_values(proof))
    for root in lay["fri_commitments"]:
        ch.mix(root)
        ch.draw()
    at = next(pos for pos, _, what in lay["prefixes"] if what == "last_layer_poly")
    F.mix_last(ch, w[at + 2:at + 2 + 4 * (1 << lay["log_last"])].reshape(-1, 4))
    out = np.zeros(16, np.uint32)
    out[:8] = ch.digest
    return out


def stored_nonce(proof, ob):
    pos = 4 * ob.proof_layout(proof)["nonce_word"]
    return int.from_bytes(proof[pos:pos + 8], "little")
