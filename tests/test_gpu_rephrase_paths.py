"""`rephrase_weight > 0` on the fast paths (include/anyref_hip.h `anyref_set_rephrase_paths`): the fused launch
pair in the tail of a plain call, under early [SEG] masks, with drafts and inside image sessions.

Setup everywhere: `config_tiny()` with rephrase_weight 0.5 and a first [SEG] at answer index >= 2 in every row that is rephrased,
so that every span [s0, e0) holds at least two rows: with one row `w_j / tot` is 1 whatever the attention pass computes, and a
wrong key pointer, query row, scale or a lost `keep_q` could not show.  The one-row rig (`Rig(B = 1)`, seed 7) gets that from
`rig_seg` as it stands (answer [983, 186, 82, ...], [SEG] = 82 at index 2); `own_seg` states the rule on the handle's own answer (the
16-bit modes need not emit the oracle's ids) and asserts it.  The two-row rig uses seed 3, whose rows both hold such an id.  In
the session rig `rig_seg`'s id is query 0's first answer token as well (an empty span), so the session tests ask queries 2, 3, 4,
whose first [SEG]s sit at answer indices 2, 4, 2.  The bounds are the project's own: 2e-5 * max(1, |mask|max) between two f32 orders of one sum
(tests/test_gpu_e2e.py test_early_seg_masks), MASK_TOL against the oracle and between a session and plain calls."""
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from anyref_amd.config import config_tiny  # noqa: E402
from oracle import anyref_oracle as O  # noqa: E402
from test_gpu_draft import Rig, extend_case, same_result  # noqa: E402
from test_gpu_e2e import MASK_TOL  # noqa: E402
from test_gpu_session import SRig, bitwise, hidden_rows  # noqa: E402

T_NEW = 6


def rcfg():
    cfg = config_tiny()
    cfg.rephrase_weight = 0.5
    return cfg


def pick_seg(answers, prompts):
    """-> (id, first index per row or None): the id that is new at an answer index >= 2 in the most rows (then: earliest in the first
    of them), occurs in no prompt and has no first occurrence before index 2 in any row"""
    old = set(int(t) for p in prompts for t in p)
    best = None
    for t in sorted({t for a in answers for t in a} - old):
        first = [a.index(t) if t in a else None for a in answers]
        if any(f is not None and f < 2 for f in first):
            continue
        key = (-sum(f is not None for f in first), min(f for f in first if f is not None), t)
        if best is None or key < best[0]:
            best = (key, t, first)
    assert best, f"no id of {answers} is new at an answer index >= 2"
    return best[1], best[2]


def own_seg(r):
    """name an id of the handle's own answers [SEG] so that every first [SEG] has a span of at least two rows; -> spans per row"""
    seg, first = pick_seg(r.gen()["new"], [i.tolist() for i in r.ids])
    r.m.set_seg_token_idx(int(seg))
    assert first[0] is not None and all(f is None or f >= 2 for f in first), first
    return first


def reassoc(a, b, what):
    """masks and low-res logits of two paths over the same stored operands: the f32-reassociation bound"""
    assert a["masks"] is not None and b["masks"] is not None, what
    scale = max(max(t.abs().max().item() for t in a["masks"] if t.numel()), 1.0)
    for x, y in zip(a["masks"], b["masks"]):
        assert x.shape == y.shape, what
        if x.numel():
            err = (x - y).abs().max().item()
            assert err <= 2e-5 * scale, (what, err, scale)
    err = (a["low"] - b["low"]).abs().max().item()
    assert err <= 2e-5 * scale, (what, "low-res", err, scale)


def on_off(r, what, rows):
    """the same call with the switch off and on, early tail off: ids and hidden rows bit for bit (rephrasing never feeds the
    decode), masks within the reassociation bound; -> (off, on)"""
    r.m.set_early_tail(False)
    r.m.set_rephrase_paths(False)
    off = r.gen()
    r.m.set_rephrase_paths(True)
    on = r.gen()
    assert torch.equal(on["ids"], off["ids"]), what
    for b, n in enumerate(rows):
        assert torch.equal(on["hidden"][b, :n], off["hidden"][b, :n]), f"{what}: hidden rows of row {b}"
    reassoc(on, off, what)
    assert r.m.early_masks_done == 0
    return off, on


# ----------------------------------------------------------------------------------------------------------------------
# 1. plain call, switch on against off
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B", [("parity", 1), ("parity", 2), ("parity16", 1), ("perf", 1), ("perf_f16", 1)])
def test_plain_call_switch_on_equals_off(mode, B):
    r = Rig(mode, B, cfg=rcfg(), seed=7 if B == 1 else 3)
    first = own_seg(r)
    if B == 2:
        assert None not in first, "both rows of this rig are rephrased: two items in one launch pair"
    rows = [s + T_NEW - 1 for s in r.slen]
    off, on = on_off(r, f"{mode} B={B}", rows)
    for b in range(B):
        assert first[b] is None or on["new"][b].index(r.m.cfg.seg_token_idx) == first[b] >= 2
    # the low-res logits hold what was computed whatever the batch rule makes of the masks: the rephrased slot is not zero
    assert on["low"][0, 0].abs().max().item() > 0
    if mode == "parity" and B == 1:
        with torch.no_grad():
            ref = O.anyref_generate(r.sd, r.m.cfg, r.clip, r.ids, r.sam, r.sizes, r.H, r.W, max_new_tokens=T_NEW, eos=False)
        assert on["ids"][0].tolist() == ref["output_ids"][0].tolist()
        err = (on["masks"][0] - ref["pred_masks"][0]).abs().max().item()
        assert err <= MASK_TOL, f"switch on vs oracle: mask err {err}"


def test_plain_call_llama_7b_widths():
    """dim 4096, 32 heads (hd 128), two layers, max_seq 512, perf: sixteen lanes per key row, 300+ keys"""
    cfg, sd = extend_case(1)[:2]
    cfg = dataclasses.replace(cfg, rephrase_weight=0.5)
    r = Rig("perf", 1, cfg=cfg, sd=sd, seed=41, T=4)
    own_seg(r)
    on_off(r, "perf, 7B widths", [r.slen[0] + 3])


# ----------------------------------------------------------------------------------------------------------------------
# 2. early masks with rephrasing
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity", "perf"])
def test_early_masks_with_rephrase(mode):
    r = Rig(mode, 1, cfg=rcfg(), seed=7)
    own_seg(r)
    r.m.set_rephrase_paths(True)
    res, done = [], []
    for early in (False, True):
        r.m.set_early_tail(early)
        res.append(r.gen())
        done.append(r.m.early_masks_done)
    a, b = res
    n = r.slen[0] + T_NEW - 1
    assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["hidden"][0, :n], b["hidden"][0, :n])
    assert a["masks"][0].shape == b["masks"][0].shape and a["masks"][0].shape[0] >= 1
    reassoc(a, b, f"{mode}: early on vs off")
    assert done[0] == 0 and done[1] >= 1, done
    # the switch off: rephrasing keeps the early path off, as before
    r.m.set_rephrase_paths(False)
    c = r.gen()
    assert r.m.early_masks_done == 0
    reassoc(c, a, f"{mode}: switch off")


# ----------------------------------------------------------------------------------------------------------------------
# 3. sessions
# ----------------------------------------------------------------------------------------------------------------------
QS = [2, 3, 4]          # the session rig's queries with a first [SEG] at answer index 2, 4, 2


@functools.lru_cache(maxsize=None)
def rsrig(mode):
    r = SRig(mode, cfg=rcfg())
    r.m.set_rephrase_paths(True)
    from test_gpu_session import HH, WW
    r.m_hw = (HH[0], WW[0])
    for q in QS:       # the first [SEG] of each of these answers has a span of two rows or more
        assert r.plain(q)["nseg"][0] >= 1 and r.new(r.plain(q), 0, q).index(r.m.cfg.seg_token_idx) >= 2, (q, r.new(r.plain(q), 0, q))
    print(f"[{mode}] plain answers {[r.new(r.plain(q), 0, q) for q in range(5)]}, [SEG]s {[r.plain(q)['nseg'][0] for q in range(5)]}")
    return r


@pytest.mark.parametrize("mode", ["parity", "parity16"])
@pytest.mark.parametrize("Q", [1, 2, 3])
def test_session_with_rephrase_equals_plain_calls(mode, Q):
    """(every row of the call is an item of one launch pair, with spans of 2, 4 and 2 rows)"""
    r = rsrig(mode)
    r.m.set_rephrase_paths(True)
    qs = QS[:Q]
    with r.open() as sess:
        a = r.ask(sess, qs)
    assert a["passes"] == 0 and a["offered"] == [0] * Q
    r.check(a, qs, f"{mode} Q={Q}")
    assert a["masks"] is not None and len(a["masks"]) == Q
    for b in range(Q):
        assert a["masks"][b].shape[0] == a["nseg"][b]
    assert a["masks"][0].shape[0] >= 1 and a["masks"][0].abs().max().item() > 0


@pytest.mark.parametrize("mode", ["parity", "parity16"])
def test_session_rows_without_a_seg_get_empty_masks(mode):
    """Session rows are independent queries: a row without a [SEG] returns an empty mask tensor and the other rows keep their
    masks -- not the reference's all-zero masks for a batched call with fewer [SEG]s than samples.  The [SEG] id is chosen here
    among the ids of one query's answer (first at index 2 or later: a span of two rows at least) that two other answers lack."""
    r = rsrig(mode)
    r.m.set_rephrase_paths(True)
    new = [r.new(r.plain(q), 0, q) for q in range(5)]
    prompt = set(r.prefix.tolist()) | {t for s_ in r.suffixes for t in s_.tolist()}
    pick = None
    for qa in range(5):
        for t in new[qa][2:]:
            without = [q for q in range(5) if q != qa and t not in new[q]]
            if t not in prompt and new[qa].index(t) >= 2 and len(without) >= 2:
                pick = (qa, t, without[:2])
                break
        if pick:
            break
    assert pick, f"no id is new at index >= 2 of one answer and missing from two others: {new}"
    qa, seg, (q1, q2) = pick
    rigged = r.m.cfg.seg_token_idx
    try:
        r.m.set_seg_token_idx(seg)
        r._plain.clear()
        for Q, qs in ((2, [qa, q1]), (3, [q1, qa, q2])):
            for q in qs:
                r.plain(q)
            with r.open() as sess:
                a = r.ask(sess, qs)
            r.check(a, qs, f"{mode} Q={Q}, rows without a [SEG]")
            assert a["masks"] is not None and len(a["masks"]) == Q
            for b, q in enumerate(qs):
                if q == qa:
                    assert a["nseg"][b] >= 1 and a["masks"][b].shape[0] == a["nseg"][b] and a["masks"][b].abs().max().item() > 0
                else:
                    assert a["nseg"][b] == 0 and tuple(a["masks"][b].shape) == (0, r.m_hw[0], r.m_hw[1]), "an empty mask tensor"
    finally:
        r.m.set_seg_token_idx(rigged)
        r._plain.clear()
        for q in range(5):
            r.plain(q)


@pytest.mark.parametrize("mode", ["parity", "parity16"])
def test_later_session_calls_equal_a_fresh_session(mode):
    r = rsrig(mode)
    r.m.set_rephrase_paths(True)
    with r.open() as sess:
        r.ask(sess, [2])
        a3 = r.ask(sess, [2, 3, 4])
        b2 = r.ask(sess, [3, 0])
    with r.open() as sess:
        a3f = r.ask(sess, [2, 3, 4])
    with r.open() as sess:
        b2f = r.ask(sess, [3, 0])
    bitwise(a3, a3f, "Q = 3 after Q = 1", hidden_rows(r, [2, 3, 4], a3))
    bitwise(b2, b2f, "Q = 2 after Q = 3", hidden_rows(r, [3, 0], b2))


# ----------------------------------------------------------------------------------------------------------------------
# 4. drafts
# ----------------------------------------------------------------------------------------------------------------------
def test_drafts_with_rephrase():
    """Between the undrafted call and each drafted one the handle answers ANOTHER prompt of the same length, which leaves other
    queries in the kept-query rows behind the prompt: the drafted call's [SEG] query is then provably its own -- written by the
    verification pass (true draft) or by the step that redoes a rejected row (wrong draft) -- not a leftover of the call before."""
    r = Rig("parity", 1, cfg=rcfg(), seed=7)
    first = own_seg(r)
    r.m.set_rephrase_paths(True)
    other = r.padded.clone()
    other[0, 2:] = other[0, 2:].roll(1)

    def overwrite():
        ids, _, _ = r.m.generate(r.clip, other, r.sam, r.sizes, r.H, r.W, max_new_tokens=T_NEW, attention_masks=r.mask)
        assert ids[0, other.shape[1]:].tolist() != p["new"][0], "another prompt, another answer: other queries in those rows"

    p = r.gen()
    assert p["masks"] is not None and p["new"][0].index(r.m.cfg.seg_token_idx) == first[0] >= 2
    true = p["new"][0][:5]
    rows = [r.slen[0] + 5]
    overwrite()
    d = r.gen(draft=[true])                       # the [SEG] row's query comes from the verification pass
    assert d["offered"] == [5] and d["accepted"] == [5] and d["passes"] == 1 and d["steps"] == 0, d
    same_result(d, p, "true draft", rows=rows)
    wrong = list(true)
    wrong[1] = (wrong[1] + 1) % r.cfg.llm.vocab
    overwrite()
    w = r.gen(draft=[wrong])                      # ... and here from a later step: the pass's row was rejected
    assert w["offered"] == [5] and w["accepted"] == [1] and w["passes"] == 1 and w["steps"] == 4, w
    same_result(w, p, "draft wrong at 1", rows=rows)


def test_drafts_with_rephrase_inside_a_session():
    """Query 2 (suffix of 5 ids, first [SEG] at answer index 2: its query is row P + 6).  Before each drafted call the session
    answers query 4 (suffix of 3 ids: its decode steps write the kept queries of rows P + 3 .. P + 7), so row P + 6 holds another
    query until the drafted call's pass, or its later step, writes it."""
    r = rsrig("parity")
    r.m.set_rephrase_paths(True)
    q = 2
    assert len(r.suffixes[q]) == 5 and len(r.suffixes[4]) == 3
    true = [r.new(r.plain(q), 0, q)[:5]]
    with r.open() as sess:
        p = r.ask(sess, [q])
        r.ask(sess, [4])
        d = r.ask(sess, [q], draft=true)
        assert d["offered"] == [5] and d["accepted"] == [5] and d["passes"] == 1 and d["steps"] == 0, d
        r.check(d, [q], "true draft")
        same_result(d, p, "true draft vs no draft", rows=hidden_rows(r, [q], p))
        wrong = [list(true[0])]
        wrong[0][1] = (wrong[0][1] + 1) % r.cfg.llm.vocab
        r.ask(sess, [4])
        w = r.ask(sess, [q], draft=wrong)
        assert w["offered"] == [5] and w["accepted"] == [1] and w["passes"] == 1 and w["steps"] == 4, w
        r.check(w, [q], "draft wrong at 1")
        same_result(w, p, "wrong draft vs no draft", rows=hidden_rows(r, [q], p))


# ----------------------------------------------------------------------------------------------------------------------
# 5. the switch turned off again
# ----------------------------------------------------------------------------------------------------------------------
def test_switch_off_restores_the_refusal_and_the_ignored_draft():
    r = rsrig("parity")
    r.m.set_rephrase_paths(True)
    with r.open() as sess:
        on = r.ask(sess, [2])
        r.m.set_rephrase_paths(False)
        try:
            with pytest.raises(RuntimeError, match="rephrase_weight > 0"):
                r.ask(sess, [2])
        finally:
            r.m.set_rephrase_paths(True)
        bitwise(r.ask(sess, [2]), on, "after the refusal", hidden_rows(r, [2], on))
    g = Rig("parity", 1, cfg=rcfg(), seed=7)
    own_seg(g)
    g.m.set_rephrase_paths(True)
    p = g.gen()
    assert g.gen(draft=[p["new"][0][:5]])["offered"] == [5]
    g.m.set_rephrase_paths(False)
    d = g.gen(draft=[p["new"][0][:5]])
    assert d["offered"] == [0] and d["passes"] == 0 and d["steps"] == 5
    reassoc(d, p, "switch off")
