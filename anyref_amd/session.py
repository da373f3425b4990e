"""Host rules of image sessions (include/anyref_hip.h `anyref_session_open` / `anyref_session_generate`) in
plain Python: what a prefix must look like and how the rows a caller hands to `sess.generate` are cut into the suffixes the
backend prefills.  Nothing here touches the GPU; `model.image_session` uses these functions and the CPU tests hold them to
known answers.

Vocabulary: the prefix is the start every prompt about one image shares, up to and INCLUDING the image placeholder (the
reference's prompts are `system prompt + <image> + question`, so that is `system prompt + <image>`); a suffix is what follows
the placeholder in one prompt.
"""
from __future__ import annotations

from typing import List, Sequence

from .config import IMAGE_TOKEN_INDEX


def check_prefix(prefix_ids: Sequence[int]) -> List[int]:
    """-> the prefix as a list of ints.  It must end with the image placeholder and hold it exactly once."""
    p = [int(v) for v in prefix_ids]
    n = p.count(IMAGE_TOKEN_INDEX)
    if n == 0:
        raise ValueError("session prefix holds no image placeholder (it must end with one)")
    if n > 1:
        raise ValueError(f"session prefix holds {n} image placeholders (exactly one, at its end)")
    if p[-1] != IMAGE_TOKEN_INDEX:
        raise ValueError("session prefix must END with the image placeholder: what follows it belongs to the queries")
    return p


def has_prefix(row: Sequence[int], prefix: Sequence[int]) -> bool:
    """whether `row` begins with the whole prefix, placeholder included"""
    k = len(prefix)
    return len(row) >= k and [int(v) for v in row[:k]] == [int(v) for v in prefix]


def cut_rows(rows: Sequence[Sequence[int]], prefix: Sequence[int]) -> List[List[int]]:
    """The suffix of every row.  A row without an image placeholder is a suffix already.  A row with one is a full prompt as
    the reference's data loader produces it: it must begin with the session's prefix, up to and including the placeholder,
    and is cut there; one that does not (another system prompt, another image position, a second placeholder) raises and
    names the row.  Every suffix holds at least one id."""
    out = []
    for b, r in enumerate(rows):
        r = [int(v) for v in r]
        n = r.count(IMAGE_TOKEN_INDEX)
        if n > 1:
            raise ValueError(f"row {b}: {n} image placeholders in one prompt")
        if n == 1:
            if not has_prefix(r, prefix):
                raise ValueError(f"row {b} does not begin with the session's prefix ({len(prefix)} ids up to and including "
                                 "the image placeholder): it asks about another image or under another system prompt")
            r = r[len(prefix):]
        if not r:
            raise ValueError(f"row {b}: nothing follows the session's prefix")
        out.append(r)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Session pools (include/anyref_hip.h `anyref_session_pool_reserve` / `_store` / `_generate_pooled`): the host
# rules of `model.session_pool` -- which slot a key gets, who is evicted, how a list of (session, prompt) items is cut into
# calls and which cache row each item is given.  Plain Python, no GPU.
# ----------------------------------------------------------------------------------------------------------------------
def cut_rows_each(rows: Sequence[Sequence[int]], prefixes: Sequence[Sequence[int]]) -> List[List[int]]:
    """`cut_rows` with one prefix per row (row b is about the session whose prefix is prefixes[b]); an error names the row
    by its index in `rows`."""
    if len(rows) != len(prefixes):
        raise ValueError(f"{len(rows)} rows but {len(prefixes)} sessions: one session per row")
    out = []
    for b, (r, p) in enumerate(zip(rows, prefixes)):
        try:
            out.append(cut_rows([r], p)[0])
        except ValueError as e:
            raise ValueError(str(e).replace("row 0", f"row {b}", 1)) from None
    return out


class SlotTable:
    """key -> slot of a pool with `n_slots` slots, least-recently-used eviction and a generation counter per slot.

    A generation names one stay of one image in one slot: it is bumped whenever the slot's content is replaced (another key
    evicts it, or the same key is opened again) and when the slot is closed, so a session object that remembers
    (slot, generation) can tell that it has been evicted, replaced or closed."""

    def __init__(self, n_slots: int):
        if n_slots < 1:
            raise ValueError("a pool needs at least one slot")
        self.n_slots = int(n_slots)
        self._slot = {}                    # key -> slot
        self._order = []                   # keys, least recently used first
        self.gens = [0] * self.n_slots

    def __len__(self):
        return len(self._slot)

    def __contains__(self, key):
        return key in self._slot

    def lru_order(self) -> list:
        """the keys held, least recently used first"""
        return list(self._order)

    def slot_of(self, key):
        """the key's slot or None; does not count as a use"""
        return self._slot.get(key)

    def touch(self, key) -> None:
        """`key` was used: it becomes the most recently used"""
        if key in self._slot:
            self._order.remove(key)
            self._order.append(key)

    def assign(self, key):
        """-> (slot, evicted key or None) for a key that is about to be (re)opened.  A key already held keeps its slot; else the
        lowest free slot; else the least recently used key is evicted and its slot taken.  The slot's generation is bumped and
        the key becomes the most recently used."""
        evicted = None
        if key in self._slot:
            slot = self._slot[key]
            self._order.remove(key)
        else:
            free = sorted(set(range(self.n_slots)) - set(self._slot.values()))
            if free:
                slot = free[0]
            else:
                evicted = self._order.pop(0)
                slot = self._slot.pop(evicted)
            self._slot[key] = slot
        self._order.append(key)
        self.gens[slot] += 1
        return slot, evicted

    def release(self, key):
        """close `key`: -> its slot (now free, generation bumped), or None if the key is not held"""
        if key not in self._slot:
            return None
        slot = self._slot.pop(key)
        self._order.remove(key)
        self.gens[slot] += 1
        return slot


def chunk_calls(n_items: int, max_batch: int) -> List[List[int]]:
    """item indices cut, in the caller's order, into calls of at most max_batch rows: all calls full but the last"""
    if max_batch < 1:
        raise ValueError("max_batch must be >= 1")
    return [list(range(i, min(i + max_batch, n_items))) for i in range(0, n_items, max_batch)]


def place_rows(tags: Sequence, held: Sequence) -> List[int]:
    """The cache row of every item of one call.  tags[i] is what item i needs in its row (a (slot, generation) pair; any
    hashable), held[r] what cache row r holds from the call before (None: nothing known).  -> rows, a permutation of
    range(len(tags)) with rows[i] the row of item i, that puts as many items as possible into a row that already holds their
    tag (those rows' gathers are skipped); the other items fill the remaining rows in the caller's order."""
    n = len(tags)
    rows = [-1] * n
    taken = [False] * n
    for r in range(min(n, len(held))):
        if held[r] is None:
            continue
        for i in range(n):
            if rows[i] < 0 and tags[i] == held[r]:
                rows[i] = r
                taken[r] = True
                break
    free = [r for r in range(n) if not taken[r]]
    for i in range(n):
        if rows[i] < 0:
            rows[i] = free.pop(0)
    return rows


def plan_calls(tags: Sequence, max_batch: int, held: Sequence = ()) -> List[List[int]]:
    """`chunk_calls` and `place_rows` together: -> one list per call, entry r of it the index of the item that goes into cache
    row r.  `held` is what the cache rows hold before the first call; after a call, row r holds the tag of its item (rows the
    call did not use keep what they held)."""
    held = list(held) + [None] * max(0, max_batch - len(held))
    calls = []
    for chunk in chunk_calls(len(tags), max_batch):
        rows = place_rows([tags[i] for i in chunk], held)
        order = [0] * len(chunk)
        for j, r in enumerate(rows):
            order[r] = chunk[j]
            held[r] = tags[chunk[j]]
        calls.append(order)
    return calls


def default_max_prefix_rows(llm_max_seq: int, n_patches: int) -> int:
    """rows a pool slot reserves per layer when the caller names none: llm_max_seq - 2 (the longest prefix a session can open
    with) capped at the image rows plus 128 ids of system prompt -- the reference's prompts put ~35 ids in front of the image,
    and every reserved row costs 2 * layers * llm_dim cache elements per slot."""
    return max(1, min(int(llm_max_seq) - 2, int(n_patches) - 1 + 128))
