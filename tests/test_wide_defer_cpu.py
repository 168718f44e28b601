"""No GPU: a model of the deferred insertion of csrc/scan_wide.hip's split-list forms (header: "Deferred insertion").

One lane pair keeps a K-slot list, ranks 0 .. K/2 - 1 in the lower half and K/2 .. K - 1 in the upper one; both halves insert by
``insert_shift`` exactly as the kernel does (strict >, every beaten slot moves down one place), the upper half inserting what the
lower half pushes out.  ``immediate`` runs that chain on every tile.  ``deferred`` keeps ``depth`` pending tiles per pair and a
bound thr (the upper half's last slot after the last flush); a tile is a candidate where x > thr, and ALL pairs of a wave flush
when any of them has a candidate and no free pending slot -- the wave-uniform branch of the kernel -- so every sequence is run
with 1 .. 32 pairs sharing that decision, the other pairs on other kinds of sequence.  Both must leave the same (score, row) lists,
bit for bit, NaN payloads aside (a NaN never enters either list)."""
import numpy as np
import pytest

NEG = np.float32(-np.inf)
TILE = 64


def _insert_shift(ts, tr, x, v, vr):
    for j in range(len(ts)):
        c = bool(x > ts[j])
        s_old, r_old = ts[j], tr[j]
        if c:
            ts[j], tr[j] = v, vr
            v, vr = s_old, r_old


class Pair:
    def __init__(self, K):
        kl = K // 2
        self.lo_s, self.lo_r = [NEG] * kl, [-1] * kl
        self.up_s, self.up_r = [NEG] * kl, [-1] * kl
        self.pend, self.thr = [], NEG

    def chain(self, x, xr):
        """the kernel's pair_insert: the lower half's last slot as it stands goes to the upper half"""
        ps, prow = self.lo_s[-1], self.lo_r[-1]
        _insert_shift(self.lo_s, self.lo_r, x, x, xr)
        c = bool(x > ps)
        _insert_shift(self.up_s, self.up_r, x, ps if c else x, prow if c else xr)

    def flush(self, depth):
        for j in range(depth):      # the kernel runs the chain on every pending slot, empty ones included
            x, xr = self.pend[j] if j < len(self.pend) else (NEG, -1)
            self.chain(x, xr)
        self.pend = []
        self.thr = self.up_s[-1]

    def lists(self):
        return self.lo_s + self.up_s, self.lo_r + self.up_r


def immediate(seqs, K):
    pairs = [Pair(K) for _ in seqs]
    for p, seq in zip(pairs, seqs):
        for i, x in enumerate(seq):
            p.chain(x, i * TILE)
    return [p.lists() for p in pairs], sum(len(s) for s in seqs)


def deferred(seqs, K, depth):
    """all sequences have one length: the tiles of one wave's stream; returns the lists and the number of flushes"""
    pairs = [Pair(K) for _ in seqs]
    flushes = 0
    for i in range(len(seqs[0])):
        xs = [seq[i] for seq in seqs]
        if any(bool(x > p.thr) and len(p.pend) == depth for p, x in zip(pairs, xs)):
            flushes += 1
            for p in pairs:
                p.flush(depth)
        for p, x in zip(pairs, xs):
            if bool(x > p.thr):
                p.pend.append((x, i * TILE))
    for p in pairs:
        p.flush(depth)
    return [p.lists() for p in pairs], flushes + 1


N = 150      # tiles per stream: several times K, so most tiles are skipped late in the stream


def _seq(kind, K, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        s = rng.standard_normal(N)
    elif kind == "ascending":
        s = np.sort(rng.standard_normal(N))
    elif kind == "descending":
        s = np.sort(rng.standard_normal(N))[::-1]
    elif kind == "constant":
        s = np.full(N, 0.25)
    elif kind == "blocks":      # blocks of equal scores, falling then rising: the K-th place falls inside a block
        levels = np.concatenate([np.arange(10, 0, -1), np.arange(1, 12)]) * 0.125
        s = np.resize(np.repeat(levels, max(K // 3, 1) + 1), N)
    elif kind == "short":       # fewer finite tiles than K: the rest of the stream is empty (-inf, as rows past the end score)
        s = np.full(N, -np.inf)
        s[:K - 5] = rng.standard_normal(K - 5)
    elif kind == "nan_inf":
        s = rng.standard_normal(N)
        s[rng.integers(0, N, N // 6)] = np.nan
        s[rng.integers(0, N, N // 6)] = -np.inf
        s[3], s[N - 2] = np.nan, np.inf
    else:
        raise ValueError(kind)
    return [np.float32(v) for v in s]


KINDS = ("random", "ascending", "descending", "constant", "blocks", "short", "nan_inf")


def _bits(lists):
    s, r = lists
    return np.array(s, np.float32).view(np.int32).tolist(), list(r)


@pytest.mark.parametrize("n_pairs", [1, 2, 3, 8, 32])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("K", [24, 32])
def test_deferred_lists_are_the_immediate_lists(K, depth, kind, n_pairs):
    k0 = KINDS.index(kind)
    seqs = [_seq(KINDS[(k0 + p) % len(KINDS)] if p % 3 else kind, K, seed=100 * k0 + p) for p in range(n_pairs)]
    want, _ = immediate(seqs, K)
    got, flushes = deferred(seqs, K, depth)
    for p in range(n_pairs):
        assert _bits(got[p]) == _bits(want[p]), (kind, p)
    s, r = want[0]
    fin = [v for v in s if v > NEG]
    assert fin == sorted(fin, reverse=True) and len(set(x for x in r if x >= 0)) == len([x for x in r if x >= 0])
    assert flushes <= N + 1


def test_the_pending_slot_halves_the_chain_runs_on_random_streams():
    """the reason for the slot: 32 pairs of a wave, 610 iid tiles, K = 24 -- a wave-wide skip alone (depth 0: flush whenever any
    pair has a candidate) runs the chain on about nine tiles in ten, one pending slot on about half of them"""
    rng = np.random.default_rng(5)
    seqs = [[np.float32(v) for v in rng.standard_normal(610)] for _ in range(32)]
    want, _ = immediate(seqs, 24)
    got, flushes = deferred(seqs, 24, 1)
    assert [_bits(x) for x in got] == [_bits(x) for x in want]
    assert 0.35 * 610 < flushes < 0.60 * 610, flushes
