"""Host rules of session pools (anyref_amd/session.py) and the C-ABI's new entries, without a GPU:

1. SlotTable: lowest free slot first, least-recently-used eviction, a key keeps its slot, generations bump on replace and close;
2. chunk_calls / place_rows / plan_calls: calls of at most max_batch rows in the caller's order, rows placed where their image
   already sits; 3. cut_rows_each names the offending row; 4. the new symbols in the header, the ctypes table and the library.
"""
import os
import re

import pytest

from anyref_amd.config import IMAGE_TOKEN_INDEX
from test_cpu_host import _build
from anyref_amd.session import (SlotTable, chunk_calls, cut_rows_each, default_max_prefix_rows, place_rows, plan_calls)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("anyref_session_pool_reserve", "anyref_session_store", "anyref_session_generate_pooled", "anyref_session_slot_close",
       "anyref_session_pool_stats", "anyref_op_kv_gather")


# ----------------------------------------------------------------------------------------------------------------------
# 1. key -> slot, LRU, generations
# ----------------------------------------------------------------------------------------------------------------------
def test_lru_eviction_order():
    t = SlotTable(3)
    assert [t.assign(k) for k in "abc"] == [(0, None), (1, None), (2, None)]
    assert t.lru_order() == ["a", "b", "c"] and len(t) == 3
    t.touch("a")                                   # a was asked about: b is the oldest now
    assert t.lru_order() == ["b", "c", "a"]
    assert t.assign("d") == (1, "b")               # b's slot, b evicted
    assert t.assign("e") == (2, "c")
    assert t.assign("f") == (0, "a")
    assert t.lru_order() == ["d", "e", "f"] and "a" not in t and t.slot_of("a") is None
    t.touch("nobody")                              # a key that is not held: nothing happens
    assert t.lru_order() == ["d", "e", "f"]
    with pytest.raises(ValueError):
        SlotTable(0)


def test_key_reuse_and_generations():
    t = SlotTable(2)
    assert t.gens == [0, 0]
    assert t.assign("a") == (0, None) and t.gens == [1, 0]
    assert t.assign("b") == (1, None) and t.gens == [1, 1]
    assert t.assign("a") == (0, None), "a key that is opened again keeps its slot and evicts nobody"
    assert t.gens == [2, 1], "... under a new generation"
    assert t.lru_order() == ["b", "a"]
    assert t.assign("c") == (1, "b") and t.gens == [2, 2], "replace bumps the generation"
    assert t.release("a") == 0 and t.gens == [3, 2], "close bumps it too"
    assert t.release("a") is None and t.gens == [3, 2]
    assert t.assign("d") == (0, None), "the freed slot is taken before anybody is evicted"
    assert t.gens == [4, 2] and t.lru_order() == ["c", "d"]
    assert t.slot_of("c") == 1 and t.lru_order() == ["c", "d"], "slot_of is no use"


# ----------------------------------------------------------------------------------------------------------------------
# 2. chunking and row placement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", [1, 3, 4])
def test_chunking(mb):
    assert chunk_calls(0, mb) == []
    assert chunk_calls(1, mb) == [[0]]
    assert chunk_calls(mb, mb) == [list(range(mb))]
    assert chunk_calls(mb + 1, mb) == [list(range(mb)), [mb]]
    for n in (1, mb, mb + 1, 3 * mb + 2):
        calls = chunk_calls(n, mb)
        assert [i for c in calls for i in c] == list(range(n)), "every item once, in the caller's order"
        assert all(1 <= len(c) <= mb for c in calls) and all(len(c) == mb for c in calls[:-1])
    with pytest.raises(ValueError):
        chunk_calls(3, 0)


def test_row_placement_maximises_skipped_gathers():
    # nothing known: the caller's order
    assert place_rows(["a", "b", "c"], [None] * 3) == [0, 1, 2]
    assert place_rows(["a", "b", "c"], []) == [0, 1, 2]
    # the same assignment again: every row stays where it is
    assert place_rows(["a", "b", "c"], ["a", "b", "c"]) == [0, 1, 2]
    # the same images in another order: every item goes to the row that holds its image
    assert place_rows(["c", "a", "b"], ["a", "b", "c"]) == [2, 0, 1]
    # one image twice, held twice
    assert place_rows(["a", "b", "a"], ["a", "a", "b"]) == [0, 2, 1]
    # one image twice, held once: one match, the other copy fills the free row
    assert place_rows(["a", "a"], ["b", "a"]) == [1, 0]
    # a shorter call only uses rows [0, n): a match in a row beyond is no match
    assert place_rows(["c", "a"], ["a", "b", "c"]) == [1, 0]
    # the best possible count, whatever the order: sum over tags of min(items, rows holding it)
    import itertools
    for tags in itertools.product("abc", repeat=3):
        for held in itertools.product(["a", "b", "c", None], repeat=3):
            rows = place_rows(list(tags), list(held))
            assert sorted(rows) == [0, 1, 2]
            got = sum(held[r] == t for t, r in zip(tags, rows))
            best = sum(min(tags.count(x), held.count(x)) for x in "abc")
            assert got == best, (tags, held, rows)


def test_plan_calls_keeps_rows_across_calls():
    # 7 items about 3 images, max_batch 3, round-robin: after the first call every image sits in a row and stays there
    tags = ["a", "b", "c", "a", "b", "c", "a"]
    calls = plan_calls(tags, 3)
    assert calls == [[0, 1, 2], [3, 4, 5], [6]]
    assert sorted(i for c in calls for i in c) == list(range(7))
    # shifted: the second call's items are c, a, b -- each is put into the row that holds its image
    tags = ["a", "b", "c", "c", "a", "b"]
    assert plan_calls(tags, 3) == [[0, 1, 2], [4, 5, 3]]
    # what the rows held before the first call counts
    assert plan_calls(["b", "a"], 2, held=["a", "b"]) == [[1, 0]]
    # one item, max_batch items, max_batch + 1 items
    assert plan_calls(["a"], 4) == [[0]]
    assert plan_calls(list("abcd"), 4) == [[0, 1, 2, 3]]
    assert plan_calls(list("abcda"), 4) == [[0, 1, 2, 3], [4]]


# ----------------------------------------------------------------------------------------------------------------------
# 3. per-row prefix check
# ----------------------------------------------------------------------------------------------------------------------
def test_each_row_is_cut_against_its_own_prefix():
    I = IMAGE_TOKEN_INDEX
    pa, pb = [1, 5, 6, I], [1, 9, I]
    rows = [pa + [20, 21], [30], pb + [40]]
    assert cut_rows_each(rows, [pa, pb, pb]) == [[20, 21], [30], [40]]
    with pytest.raises(ValueError, match="row 2 does not begin"):
        cut_rows_each(rows, [pa, pb, pa])          # row 2 is about image b, the session given for it is a's
    with pytest.raises(ValueError, match="row 1: nothing follows"):
        cut_rows_each([pa + [20], pb], [pa, pb])
    with pytest.raises(ValueError, match="row 1: 2 image placeholders"):
        cut_rows_each([[20], pb + [I, 3]], [pa, pb])
    with pytest.raises(ValueError, match="one session per row"):
        cut_rows_each(rows, [pa, pb])


def test_default_prefix_rows():
    assert default_max_prefix_rows(512, 256) == 383   # LLaMA at 512: 255 image rows + 128 ids
    assert default_max_prefix_rows(320, 256) == 318   # the cache is the limit: llm_max_seq - 2
    assert default_max_prefix_rows(2, 1) == 1


# ----------------------------------------------------------------------------------------------------------------------
# 4. the C-ABI
# ----------------------------------------------------------------------------------------------------------------------
def test_new_entries_in_header_table_and_library():
    _build()
    from anyref_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "anyref_hip.h")).read() + open(os.path.join(ROOT, "include", "anyref_hip_ops.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in the headers"
        assert name in _lib.SYMBOLS, f"{name} is not in the ctypes table"
        assert getattr(lib, name) is not None
    # the number of arguments the table passes is the number the header declares
    for name in NEW:
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name
    assert re.search(r"#define\s+ANYREF_ABI_VERSION\s+2\b", hdr) and _lib.ABI_VERSION == 2


def test_python_surface():
    from anyref_amd.model import AnyRefForCausalLM, PooledSession, SessionPool
    assert callable(AnyRefForCausalLM.session_pool)
    for name in ("open", "get", "close", "generate", "generate_many", "stats"):
        assert callable(getattr(SessionPool, name))
    assert callable(PooledSession.check)
    from anyref_amd import parallel
    assert "pool" in parallel.__doc__
