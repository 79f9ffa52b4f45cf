"""CPU: dbaf_amd._lib.EdgeSetMemo, what lets a later call of update_inputs.assemble and vio_window.split read nothing.
No device and no library: CPU tensors carry `_version` and accept weak references."""
import gc

import pytest
import torch

from dbaf_amd import _lib
from dbaf_amd import update_inputs as ux
from dbaf_amd import vio_window as vw

KEY = (3, 5, 64)


def edge_lists(n=4, seed=0):
    return tuple(torch.arange(6, dtype=torch.int64) + 10 * seed + k for k in range(n))


@pytest.fixture
def memo():
    return _lib.EdgeSetMemo(capacity=8)


def test_hit_on_the_same_objects_versions_and_key(memo):
    L = edge_lists()
    assert memo.lookup(L, KEY) is None
    value = dict(N=7)
    memo.remember(L, KEY, value)
    assert memo.lookup(L, KEY) is value
    assert memo.lookup(tuple(L), (3, 5, 64)) is value       # an equal key, another tuple of the same tensors


@pytest.mark.parametrize("which", range(4))
def test_miss_after_an_in_place_write_to_any_one_list(memo, which):
    L = edge_lists()
    memo.remember(L, KEY, "block")
    L[which][0] = 99
    assert memo.lookup(L, KEY) is None
    memo.remember(L, KEY, "again")                           # the written set is a new edge set
    assert memo.lookup(L, KEY) == "again"


def test_miss_for_a_clone_with_equal_contents(memo):
    L = edge_lists()
    memo.remember(L, KEY, "block")
    for which in range(4):
        other = L[:which] + (L[which].clone(),) + L[which + 1:]
        assert torch.equal(other[which], L[which]) and memo.lookup(other, KEY) is None
    assert memo.lookup(L, KEY) == "block"


def test_miss_for_a_different_key(memo):
    L = edge_lists()
    memo.remember(L, KEY, "block")
    for key in ((None, 5, 64), (3, 6, 64), (3, 5, 65), (3, 5), KEY + (0,)):
        assert memo.lookup(L, key) is None
    assert memo.lookup(L, KEY) == "block"


def test_miss_with_one_more_or_one_fewer_tensor(memo):
    L = edge_lists()
    memo.remember(L, KEY, "block")
    assert memo.lookup(L[:3], KEY) is None
    assert memo.lookup(L + (L[0],), KEY) is None
    assert memo.lookup(L, KEY) == "block"


def test_the_newest_of_two_matching_entries_wins(memo):
    L = edge_lists()
    memo.remember(L, KEY, "older")
    memo.remember(L, KEY, "newer")
    assert memo.lookup(L, KEY) == "newer"


def test_an_entry_whose_tensor_was_deleted_is_gone_after_the_next_remember(memo):
    L, M, K = edge_lists(seed=1), edge_lists(seed=2), edge_lists(seed=3)
    memo.remember(L, KEY, "L")
    memo.remember(M, KEY, "M")
    assert len(memo) == 2
    keep = L[1:]
    del L
    gc.collect()
    assert len(memo) == 2                                    # (nothing prunes between remembers)
    memo.remember(K, KEY, "K")
    assert len(memo) == 2 and memo.lookup(M, KEY) == "M" and memo.lookup(K, KEY) == "K"
    assert all(x._version == 0 for x in keep)


def test_a_ninth_remember_evicts_the_oldest_and_keeps_the_other_seven(memo):
    sets = [edge_lists(seed=s) for s in range(9)]
    for s, L in enumerate(sets[:8]):
        memo.remember(L, KEY, s)
    assert len(memo) == 8 and [memo.lookup(L, KEY) for L in sets[:8]] == list(range(8))
    memo.remember(sets[8], KEY, 8)
    assert len(memo) == 8 and memo.lookup(sets[0], KEY) is None
    assert [memo.lookup(L, KEY) for L in sets[1:]] == list(range(1, 9))


def test_clear_empties_the_memo(memo):
    L, M = edge_lists(seed=1), edge_lists(seed=2)
    memo.remember(L, KEY, "L")
    memo.remember(M, KEY, "M")
    memo.clear()
    assert len(memo) == 0 and memo.lookup(L, KEY) is None and memo.lookup(M, KEY) is None
    memo.remember(L, KEY, "L again")
    assert memo.lookup(L, KEY) == "L again"


def test_the_two_modules_own_distinct_memos():
    assert isinstance(ux._MEMO, _lib.EdgeSetMemo) and isinstance(vw._MEMO, _lib.EdgeSetMemo)
    assert ux._MEMO is not vw._MEMO and ux._MEMO.capacity == vw._MEMO.capacity == 8
    L = edge_lists()
    held = (list(ux._MEMO._entries), list(vw._MEMO._entries))
    try:
        ux._MEMO.remember(L, KEY, "counts")
        assert ux._MEMO.lookup(L, KEY) == "counts" and vw._MEMO.lookup(L, KEY) is None
        vw._MEMO.clear()                                     # a report of one module's guard leaves the other's memo
        assert ux._MEMO.lookup(L, KEY) == "counts"
    finally:
        ux._MEMO._entries[:], vw._MEMO._entries[:] = held
