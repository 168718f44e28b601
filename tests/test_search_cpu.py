"""CPU: the exactness tally of rag/_search.py (numpy only) from hand-written status arrays, and the two policies the store and the
engine share."""
import numpy as np

from rag import _native as nat
from rag import _search

ST = np.array([0, 0, 1, 2, 0, 1], dtype=np.int32)


def _counts(t):
    return t["queries"], t["certified"], t["escalated"], t["unproven"], t["mode"]


def test_one_shard_escalating():
    assert _counts(_search.tally(ST, 6, 10, True, True)) == (6, 3, 2, 1, "certificate")
    assert _counts(_search.tally([ST], 6, 100, True, True)) == (6, 3, 2, 1, "certificate")


def test_one_shard_not_escalating_counts_status_1_unproven():
    assert _counts(_search.tally(ST, 6, 10, True, False)) == (6, 3, 0, 3, "certificate")


def test_two_shards_count_a_query_by_its_worst_shard():
    other = np.array([1, 0, 0, 0, 2, 1], dtype=np.int32)
    #          worst:  1  0  1  2  2  1
    assert _counts(_search.tally([ST, other], 6, 10, True, True)) == (6, 1, 3, 2, "certificate")
    assert _counts(_search.tally([ST, None, other], 6, 10, True, False)) == (6, 1, 0, 5, "certificate")


def test_no_shard_with_rows_misses_nothing():
    assert _counts(_search.tally(None, 4, 10, True, True)) == (4, 4, 0, 0, "certificate")
    assert _counts(_search.tally([None, None], 4, 10, True, True)) == (4, 4, 0, 0, "certificate")


def test_top_k_above_the_certificate_limit_is_a_rerank():
    assert _counts(_search.tally(None, 6, nat.MAX_K_CERT + 1, True, True)) == (6, 0, 0, 6, "rerank")
    assert _counts(_search.tally(ST, 6, nat.MAX_K_CERT, True, True))[4] == "certificate"


def test_unrefined_store_claims_nothing():
    assert _counts(_search.tally(ST, 6, 10, False, True)) == (0, 0, 0, 0, "slab")
    assert _counts(_search.tally(None, 6, 5000, False, False)) == (0, 0, 0, 0, "slab")


def test_a_retry_tally_replaces_the_batchs_unproven_queries():
    batch = _search.tally(ST, 6, 10, True, True)                                  # one status-2 query
    retry = _search.tally(np.array([1], dtype=np.int32), 1, 10, True, True)       # ... escalated with a longer list
    both = _search.retried_tally(batch, retry)
    assert _counts(both) == (6, 3, 3, 0, "certificate")
    assert both["certified"] + both["escalated"] + both["unproven"] == both["queries"]
    still = _search.retried_tally(batch, _search.tally(np.array([2], dtype=np.int32), 1, 10, True, True))
    assert _counts(still) == (6, 3, 2, 1, "certificate")
    total = _search.add_tallies(both, _search.tally(np.zeros(4, dtype=np.int32), 4, 10, True, True))
    assert _counts(total) == (10, 7, 3, 0, "certificate")
    assert batch == _search.tally(ST, 6, 10, True, True)                          # the inputs are left as they were


def test_policies():
    assert _search.escalates("auto", nat.SLAB_F16) and not _search.escalates("auto", nat.SLAB_I8)
    assert _search.escalates(True, nat.SLAB_I8) and not _search.escalates(False, nat.SLAB_F16)
    assert _search.first_cap(nat.EXACT_CAP, 10) == _search.first_cap(nat.EXACT_CAP, nat.MAX_K) == nat.EXACT_CAP
    assert _search.first_cap(64, 100) == 400 and _search.first_cap(64, 10) == 64
    assert _search.first_cap(nat.EXACT_CAP, nat.MAX_K_CERT) == 4 * nat.MAX_K_CERT <= nat.EXACT_MAX_CAP
