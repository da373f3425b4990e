"""Host rules of the draft-verified greedy decode (anyref_amd/draft.py: what anyref_generate does with a proposed answer before
and after its verification pass) held to hand-worked answers, and the two forms `generate(draft_ids=...)` accepts.  No GPU."""
import inspect
import os
import re

import pytest
import torch

from anyref_amd import draft as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 1000


def run_row(t0, draft, answer, max_new, eos=None, **cut):
    """One row through cut -> offered -> accept -> append, with a model whose greedy answer is `answer` whatever the prefix
    (answer[0] = t0): the pass returns p[j] = answer[j + 1] while the fed tokens match.  -> (tokens, offered, accepted)"""
    assert answer[0] == t0
    k = D.offered(t0, draft or [], D.cut_draft(draft, V, max_new, **cut))
    have, m = [], 0
    if k:
        preds = []
        for j in range(k):          # the model sees d[0 .. j]; its prediction is the answer's only while they match
            preds.append(answer[j + 1] if list(draft[: j + 1]) == answer[: j + 1] else 999)
        m, g = D.accept(t0, draft[:k], preds)
        ended = D.append_tokens(have, g, eos, max_new)
    else:
        ended = D.append_tokens(have, [t0], eos, max_new)
    i = len(have)
    while not ended:                # the one-token loop
        ended = D.append_tokens(have, [answer[i]], eos, max_new)
        i += 1
    return have, k, m


ANS = [11, 12, 13, 14, 15, 16, 17, 18]


def plain(max_new, eos=None):
    out = []
    for t in ANS[:max_new]:
        out.append(t)
        if eos is not None and t == eos:
            break
    return out


def test_all_accepted():
    got, k, m = run_row(11, ANS[:5], ANS, 6)
    assert (got, k, m) == (ANS[:6], 5, 5)              # 5 fed, 5 accepted, 6 tokens: no decode step left


def test_mismatch_at_zero_offers_nothing():
    got, k, m = run_row(11, [99, 12, 13], ANS, 6)
    assert (got, k, m) == (ANS[:6], 0, 0)


def test_mismatch_in_the_middle():
    got, k, m = run_row(11, [11, 12, 77, 14, 15], ANS, 6)
    assert (got, k, m) == (ANS[:6], 5, 2)
    assert D.accept(11, [11, 12, 77, 14, 15], [12, 13, 555, 556, 557]) == (2, [11, 12, 13])


def test_eos_inside_the_accepted_run():
    got, k, m = run_row(11, ANS[:5], ANS, 6, eos=14)
    assert got == plain(6, eos=14) == [11, 12, 13, 14] and (k, m) == (5, 5)
    have = []
    assert D.append_tokens(have, [11, 12, 14, 15], 14, 10) and have == [11, 12, 14]
    have = [1, 2]
    assert D.append_tokens(have, [3, 4, 5], None, 4) and have == [1, 2, 3, 4]
    have = [1]
    assert not D.append_tokens(have, [3], -1, 4) and have == [1, 3]


def test_draft_longer_than_max_new_tokens_minus_one():
    assert D.cut_draft(ANS, V, 6) == 5
    assert D.cut_draft(ANS, V, 1) == 0                # one new token: prefill already chose it
    assert D.cut_draft(list(range(200)), V, 500) == D.DRAFT_CAP == 64
    got, k, m = run_row(11, ANS, ANS, 4)
    assert (got, k, m) == (ANS[:4], 3, 3)


def test_invalid_ids_end_the_draft():
    assert D.cut_draft([11, 12, -1, 14], V, 10) == 2
    assert D.cut_draft([11, V, 13], V, 10) == 1
    assert D.cut_draft([V + 5], V, 10) == 0
    assert D.cut_draft([11, V - 1], V, 10) == 2
    got, k, m = run_row(11, [11, 12, -1, 14, 15], ANS, 6)
    assert (got, k, m) == (ANS[:6], 2, 2)


def test_cache_limit_for_batches():
    # slen 90, 6 new tokens, 100 cache rows: a lone row may be fed max_new - 1 = 5 tokens, a batched row max_seq - slen - max_new = 4
    assert D.cut_draft(ANS, V, 6, slen=90, max_seq=100, batch=1) == 5
    assert D.cut_draft(ANS, V, 6, slen=90, max_seq=100, batch=2) == 4
    assert D.cut_draft(ANS, V, 6, slen=94, max_seq=100, batch=2) == 0      # slen + max_new == max_seq: nothing
    assert D.cut_draft(ANS, V, 6, slen=97, max_seq=100, batch=2) == 0      # (never negative)
    # the rule's reason: the row ahead by k steps on while the slowest row takes its max_new - 1 steps
    for slen, k in ((90, 4), (80, 5)):
        last_written = slen + k + (6 - 1) - 1
        assert last_written < 100


def test_empty_and_none_rows():
    assert D.cut_draft(None, V, 6) == 0 and D.cut_draft([], V, 6) == 0
    got, k, m = run_row(11, None, ANS, 6)
    assert (got, k, m) == (ANS[:6], 0, 0)
    assert D.offered(11, [11], 0) == 0


def test_decode_steps_after_a_pass():
    assert D.decode_steps_after([6], [True], 6) == 0
    assert D.decode_steps_after([3], [False], 6) == 3
    assert D.decode_steps_after([3, 6], [False, True], 6) == 3     # ragged acceptance: the slowest row sets the count
    assert D.decode_steps_after([1, 4], [False, False], 6) == 5


def test_draft_ids_forms():
    t = torch.tensor([[5, 6, 7, -1, 9], [-1, 3, 3, 3, 3], [1, 2, 3, 4, 5]])
    assert D.normalize_drafts(t, 3) == [[5, 6, 7], [], [1, 2, 3, 4, 5]]       # [B, K]: rows end at the first negative id
    lst = [torch.tensor([5, 6]), None, [7, 8, 9]]
    assert D.normalize_drafts(lst, 3) == [[5, 6], [], [7, 8, 9]]
    assert D.normalize_drafts([[4, -1, 5], None], 2) == [[4, -1, 5], []]      # list rows are taken whole: the cut rule ends them
    assert D.cut_draft([4, -1, 5], V, 6) == 1
    with pytest.raises(ValueError):
        D.normalize_drafts([None], 2)


def test_generate_keeps_the_reference_signature_and_the_interface_is_declared():
    from anyref_amd import _lib
    from anyref_amd.model import AnyRefForCausalLM
    names = list(inspect.signature(AnyRefForCausalLM.generate).parameters)
    assert names[-1] == "draft_ids" and names[1:7] == ["clip_images", "input_ids", "sam_images", "sam_resized_sizes", "height",
                                                        "width"]
    assert inspect.signature(AnyRefForCausalLM.generate).parameters["draft_ids"].default is None
    hdr = open(os.path.join(ROOT, "include", "anyref_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "anyref_hip_ops.h")).read()
    for name, txt in (("anyref_llm_extend", hdr), ("anyref_set_draft", hdr), ("anyref_draft_stats", hdr),
                      ("anyref_op_draft_accept", ops)):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, txt), name
    assert re.search(r"#define ANYREF_ABI_VERSION 2\b", hdr) and _lib.ABI_VERSION == 2
    m = AnyRefForCausalLM.__new__(AnyRefForCausalLM)
    m._draft_policy, m._last_answers = None, [[1]]
    m.set_draft_policy("last")
    assert m._draft_policy == "last" and m._last_answers is None
    with pytest.raises(ValueError):
        m.set_draft_policy("first")
