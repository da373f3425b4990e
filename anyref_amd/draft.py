"""Host rules of the draft-verified greedy decode (include/anyref_hip.h `anyref_set_draft`), restated in
plain Python: what `anyref_generate` does with a proposed continuation before and after its one verification pass.  Nothing
here touches the GPU; `model.generate(..., draft_ids=...)` uses `normalize_drafts`, the CPU tests hold the rest to known
answers, and the GPU tests compare the backend's counters with them.

Vocabulary: t0 is the token prefill chose; a draft d proposes the generated tokens from t0 on (d[0] is compared with t0); the
pass feeds d[0 .. k) and returns p[j] = argmax of the logits behind d[j]; g[0] = t0, g[j + 1] = p[j].
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

DRAFT_CAP = 64      # tokens per row a verification pass is fed at most (ModelBase::kDraftCap)


def normalize_drafts(draft_ids, B: int) -> List[List[int]]:
    """`draft_ids` of `generate` -> B lists of ints.  Accepted: a list / tuple of B entries, each a 1-D tensor, a list of
    ints or None (no draft for that row); or a [B, K] tensor (or nested list) whose rows are cut at the first negative id."""
    two_d = hasattr(draft_ids, "dim") and draft_ids.dim() == 2
    rows = draft_ids.tolist() if hasattr(draft_ids, "tolist") else list(draft_ids)
    if len(rows) != B:
        raise ValueError(f"draft_ids has {len(rows)} rows for a batch of {B}")
    out = []
    for r in rows:
        if r is None:
            out.append([])
            continue
        r = r.tolist() if hasattr(r, "tolist") else list(r)
        r = [int(v) for v in r]
        if two_d:
            for i, v in enumerate(r):
                if v < 0:
                    r = r[:i]
                    break
        out.append(r)
    return out


def cut_draft(draft: Optional[Sequence[int]], vocab: int, max_new_tokens: int, slen: int = 0, max_seq: int = 0,
              batch: int = 1, cap: int = DRAFT_CAP) -> int:
    """Number of leading draft tokens that may be fed to the pass: the draft ends at the first id outside [0, vocab), at
    max_new_tokens - 1 tokens (the pass returns one more token than it accepts) and at `cap`; in a batch of more than one,
    also at max_seq - slen - max_new_tokens: a row that gets ahead by k tokens keeps stepping while the slowest row needs its
    max_new_tokens - 1 steps, and must stay inside the KV cache."""
    if not draft:
        return 0
    k = 0
    while k < len(draft) and 0 <= int(draft[k]) < vocab:
        k += 1
    k = min(k, max_new_tokens - 1, cap)
    if batch > 1:
        k = min(k, max_seq - slen - max_new_tokens)
    return max(k, 0)


def accept(t0: int, draft: Sequence[int], preds: Sequence[int]) -> Tuple[int, List[int]]:
    """The accept rule on one row: draft d[0 .. k) was fed, preds p[0 .. k) came back.  -> (m, g[0 .. m]): m = number of
    leading j < k with g[j] == d[j]; the m + 1 tokens are exactly what the one-token loop would have produced."""
    g = [int(t0)]
    m = 0
    while m < len(draft) and g[m] == int(draft[m]):
        g.append(int(preds[m]))
        m += 1
    return m, g


def offered(t0: int, draft: Sequence[int], k: int) -> int:
    """A row whose first token already differs from its draft offers nothing to the pass."""
    return k if k > 0 and int(draft[0]) == int(t0) else 0


def append_tokens(have: List[int], new: Sequence[int], eos: Optional[int], max_new_tokens: int) -> bool:
    """Append tokens to a row's answer as the loop does, one by one: the row ends at (and keeps) the first EOS, or when it
    holds max_new_tokens tokens.  -> whether the row has ended."""
    for t in new:
        if len(have) >= max_new_tokens:
            return True
        have.append(int(t))
        if eos is not None and eos >= 0 and int(t) == eos:
            return True
    return len(have) >= max_new_tokens


def decode_steps_after(held: Sequence[int], ended: Sequence[bool], max_new_tokens: int) -> int:
    """Decode steps the loop still launches after the pass when no row meets an EOS: every step advances every row, so the
    row that holds the fewest tokens sets the count."""
    need = [max_new_tokens - h for h, e in zip(held, ended) if not e]
    return max(need) if need else 0
