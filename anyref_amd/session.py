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
