"""CPU: nat.overfetch, the number of candidates the scan fetches for the fp32 re-rank and its certificate.

k' must never fall below top_k or above the scan kernels' MAX_K, must leave a margin (k' > top_k) wherever the cap allows
one -- with k' == top_k the re-rank only reorders the slab's own list and the certificate cannot hold -- and at top_k <= 10,
where bench.py and the shipped configs run, must keep today's lengths so those measurements do not move."""
from rag import _native as nat

NQS = (1, 8, 64, 65, 512)
ROWS = (1000, 300_000, 3_999_999, 4_000_000, 10_000_000)


def test_overfetch_stays_within_top_k_and_max_k():
    for slab in (nat.SLAB_F16, nat.SLAB_I8):
        for nq in NQS:
            for n in ROWS:
                for k in range(1, nat.MAX_K + 1):
                    kp = nat.overfetch(nq, k, 24, n, slab)
                    assert k <= kp <= nat.MAX_K, (slab, nq, n, k, kp)
                    if k < nat.MAX_K:
                        assert kp > k, f"no over-fetch margin at top_k {k} (nq {nq}, {n} rows, slab {slab}): k' = {kp}"


def test_overfetch_grows_with_top_k():
    for slab in (nat.SLAB_F16, nat.SLAB_I8):
        for nq in NQS:
            for n in ROWS:
                ks = [nat.overfetch(nq, k, 24, n, slab) for k in range(1, nat.MAX_K + 1)]
                assert ks == sorted(ks), (slab, nq, n, ks)


def test_overfetch_at_small_top_k_is_unchanged():
    """24 on fp16 shards of >= 4 M rows searched with <= 64 queries per launch, 16 otherwise and on int8 slabs."""
    for slab in (nat.SLAB_F16, nat.SLAB_I8):
        for nq in NQS:
            for n in ROWS:
                want = 24 if (slab == nat.SLAB_F16 and n >= 4_000_000 and nq <= 64) else 16
                for k in range(1, 11):
                    assert nat.overfetch(nq, k, 24, n, slab) == want, (slab, nq, n, k)
    assert nat.overfetch(64, 10, 24) == 24            # the defaults (a shard of unknown size counts as a large one)
    assert nat.overfetch(64, 10, 32, 10_000_000) == 32   # an explicit refine_overfetch is honoured where it was before
