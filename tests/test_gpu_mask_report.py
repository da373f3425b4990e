"""Mask reports through the model (include/anyref_hip.h `anyref_set_mask_reports` / `anyref_set_packed_masks` /
`anyref_mask_reports`), on the tiny config with the rig of tests/test_gpu_draft.py: masks are 300 x 241, so a row
of the packed mask ends in a partly filled word.

Everything is exact.  The rule (anyref_amd/maskreport.py) reads the `pred_masks` the same call returned, so records, stability
and packed words must EQUAL the rule's in every arithmetic mode; and the switch changes nothing a call returns, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anyref_amd.maskreport import mask_report_rule, packed_width, stability, unpack  # noqa: E402
from test_gpu_draft import Rig, T_NEW  # noqa: E402
from test_gpu_e2e import pad  # noqa: E402

MODES = ["parity", "perf"]
OFFSET = 1.0


def ptr(t):
    return C.c_void_p(t.data_ptr())


def check_entries(entries, masks, hw, what, offset=OFFSET, packed=True):
    """one entry per row against the rule on the masks the call returned for the row (masks None: no row has one)"""
    assert len(entries) == len(hw), f"{what}: {len(entries)} entries for {len(hw)} rows"
    total = 0
    for b, (e, (H, W)) in enumerate(zip(entries, hw)):
        x = np.zeros((0, H, W), dtype=np.float32) if masks is None else masks[b].detach().cpu().numpy()
        n = x.shape[0]
        total += n
        assert e["area"].shape == (n,) and e["box"].shape == (n, 4) and e["stability"].shape == (n,), f"{what}: row {b} n"
        assert e["area"].dtype == torch.int64 and e["box"].dtype == torch.int64 and e["stability"].dtype == torch.float32
        assert not e["area"].is_cuda and not e["stability"].is_cuda
        if n == 0:
            assert e["packed"] is None or e["packed"].shape[0] == 0
            continue
        rec, words = mask_report_rule(x, offset)
        for i, k in enumerate(("area", "area_hi", "area_lo", "nonfinite")):
            assert e[k].tolist() == rec[:, i].tolist(), f"{what}: row {b} {k} {e[k].tolist()}, the rule {rec[:, i].tolist()}"
        assert e["box"].tolist() == rec[:, 4:].tolist(), f"{what}: row {b} box {e['box'].tolist()}, the rule {rec[:, 4:].tolist()}"
        assert np.array_equal(e["stability"].numpy().view(np.int32), stability(rec).view(np.int32)), f"{what}: row {b} stability"
        if packed:
            p = e["packed"]
            assert p is not None and p.is_cuda and p.dtype == torch.int32 and tuple(p.shape) == (n, H, packed_width(W))
            assert np.array_equal(p.cpu().numpy().view(np.uint32), words), f"{what}: row {b} packed words"
            assert np.array_equal(unpack(p, W), x > 0)
        else:
            assert e["packed"] is None
    return total


def gen(r, **kw):
    d = r.gen(**kw)
    d["reports"] = r.m.last_mask_reports()
    return d


@functools.lru_cache(maxsize=None)
def rig(mode, B):
    """one handle with the switch on and packed masks, and its plain answer (shared, left unchanged)"""
    r = Rig(mode, B)
    r.m.set_mask_reports(True, OFFSET, packed=True)
    r.plain = gen(r)
    r.hw = list(zip(r.H, r.W))
    print(f"[{mode} B={B}] plain answer: {r.plain['new']}, masks per row {[len(t) for t in r.plain['masks']]}")
    return r


def same_answer(a, b, what):
    assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["low"], b["low"]), what
    assert (a["masks"] is None) == (b["masks"] is None)
    for x, y in zip(a["masks"] or [], b["masks"] or []):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what


# ----------------------------------------------------------------------------------------------------------------------
# off is off; the switch changes nothing a call returns
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_off_is_off_and_the_switch_changes_no_answer(mode):
    r0 = rig(mode, 1)
    r = Rig(mode, 1, cfg=r0.cfg, sd=r0.sd)
    m = r.m
    base = m.device_bytes
    with pytest.raises(RuntimeError, match="mask reports are off"):
        m.last_mask_reports()
    n, rec = torch.zeros(1, dtype=torch.int32), torch.zeros(1, T_NEW, 8, dtype=torch.int32)
    assert m.lib.anyref_mask_reports(m.h, 1, T_NEW, ptr(n), ptr(rec), None) != 0
    buf = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert m.lib.anyref_set_packed_masks(m.h, ptr(buf), 16) != 0, "a packed buffer needs the switch on"
    off = r.gen()
    with pytest.raises(RuntimeError, match="mask reports are off"):
        m.last_mask_reports()
    assert m.lib.anyref_mask_reports(m.h, 1, T_NEW, ptr(n), ptr(rec), None) != 0
    assert m.device_bytes == base, "a call with the switch off allocates nothing for it"
    m.set_mask_reports(False)
    assert m.device_bytes == base, "switching off what was never on allocates nothing"
    for step, (on, pk) in enumerate([(True, False), (True, True), (False, False), (True, True)]):
        m.set_mask_reports(on, OFFSET, packed=pk)
        if step == 0:
            assert m.device_bytes - base == 1 * T_NEW * 8 * 4, "the device records [max_batch, max_seg, 8]"
        d = r.gen()
        same_answer(d, off, f"{mode}: step {step}, switch {on}, packed {pk}")
        if on:
            assert check_entries(m.last_mask_reports(), d["masks"], r0.hw, f"{mode} step {step}", packed=pk) >= 1
        else:
            with pytest.raises(RuntimeError, match="mask reports are off"):
                m.last_mask_reports()
        m.set_graphs(False)
        try:
            e = r.gen()
        finally:
            m.set_graphs(True)
        same_answer(e, off, f"{mode}: step {step}, graphs off")
        if on:
            check_entries(m.last_mask_reports(), e["masks"], r0.hw, f"{mode} step {step}, graphs off", packed=pk)
    assert m.device_bytes - base == 1 * T_NEW * 8 * 4, "toggling allocates the records once"
    same_answer(r0.plain, off, f"{mode}: the shared rig's answer")


# ----------------------------------------------------------------------------------------------------------------------
# the records are the rule on the masks the call returned
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_batch_one_early_masks_on_and_off(mode):
    r = rig(mode, 1)
    assert r.m.early_masks_done >= 1, "the side-stream site did not run"
    assert check_entries(r.plain["reports"], r.plain["masks"], r.hw, f"{mode} early on") >= 1
    r.m.set_early_tail(False)
    try:
        d = gen(r)
        assert r.m.early_masks_done == 0
    finally:
        r.m.set_early_tail(True)
    assert torch.equal(d["ids"], r.plain["ids"])              # (the tail decodes the masks in one batch: not the same bits)
    check_entries(d["reports"], d["masks"], r.hw, f"{mode} early off")
    again = gen(r)                                              # a rerun is bit-identical
    assert r.m.early_masks_done >= 1
    for a, b in zip(again["reports"], r.plain["reports"]):
        assert all(torch.equal(a[k], b[k]) for k in ("area", "area_hi", "area_lo", "nonfinite", "box"))
        assert torch.equal(a["packed"], b["packed"])
    # another offset: the counts around it move, the rest stays
    r.m.set_mask_reports(True, 0.25, packed=True)
    try:
        d = gen(r)
        check_entries(d["reports"], d["masks"], r.hw, f"{mode} offset 0.25", offset=0.25)
    finally:
        r.m.set_mask_reports(True, OFFSET, packed=True)


@pytest.mark.parametrize("mode", MODES)
def test_ragged_batch_of_two(mode):
    r = rig(mode, 2)
    assert len(set(r.slen)) == 2, "rows of different prompt lengths"
    per_row = [len(t) for t in r.plain["masks"]]
    assert per_row[0] >= 1 and 0 in per_row, f"one row with a [SEG], one without: {per_row}"
    assert check_entries(r.plain["reports"], r.plain["masks"], r.hw, f"{mode} B=2") == sum(per_row)


@pytest.mark.parametrize("mode", MODES)
def test_seg_tail_on_canned_ids_and_one_forward(mode):
    r = rig(mode, 2)
    seg, L = r.cfg.seg_token_idx, 12
    ids = torch.full((2, L), 5, dtype=torch.long)
    ids[:, 0] = 1
    ids[0, 3] = ids[0, 7] = seg                                 # two [SEG] in one row
    ids[1, 5] = seg
    hidden = r.plain["hidden"].cuda()
    masks, nseg = r.m.seg_tail(r.sam, ids, [L, L], [2, 2], hidden, None, r.sizes, r.H, r.W)
    assert nseg.tolist() == [2, 1]
    assert check_entries(r.m.last_mask_reports(), masks, r.hw, f"{mode} seg_tail") == 3
    # one teacher-forced call over the prompt and the answer of row 0
    full = r.plain["ids"][:1, : len(r.ids[0]) + T_NEW]
    out = r.m.model_forward_new(r.clip[:1], r.sam[:1], full, full.clone(), None, r.sizes[:1], None, r.H[:1], r.W[:1],
                                _return_extras=True)
    assert check_entries(r.m.last_mask_reports(), out["pred_masks"], r.hw[:1], f"{mode} forward") >= 1


@pytest.mark.parametrize("mode", MODES)
def test_a_drafted_call(mode):
    r = rig(mode, 1)
    d = gen(r, draft=[r.plain["new"][0][:5]])
    assert d["offered"] == [5]
    assert check_entries(d["reports"], d["masks"], r.hw, f"{mode} drafted") >= 1


@pytest.mark.parametrize("mode", MODES)
def test_sessions_and_pool(mode):
    from test_gpu_session_pool import HH, QS, WW, prig
    r = prig(mode)
    m = r.m
    m.set_mask_reports(True, OFFSET, packed=True)
    try:
        padded, mask = pad([r.suffixes[0], r.suffixes[1]])
        with r.live(0) as sess:
            (ids, masks, *_), ex = sess.generate(padded, attention_masks=mask, max_new_tokens=r.T, _return_extras=True)
            rep = m.last_mask_reports()
        assert int(ex["nseg"][0]) >= 1, "image 0, query 0 was rigged to answer with a [SEG]"
        assert [len(e["area"]) for e in rep] == ex["nseg"].tolist()
        check_entries(rep, masks, [(HH[0], WW[0])] * 2, f"{mode} sess.generate, two queries")
        ks = (0, 1, 0)
        a = r.pooled(ks)
        rep = m.last_mask_reports()
        assert [len(e["area"]) for e in rep] == a["nseg"]
        assert check_entries(rep, a["masks"], [(HH[k], WW[k]) for k in ks], f"{mode} pool.generate {ks}") >= 1
        # generate_many: more items than max_batch, two calls; entries come back in the caller's item order
        order = ((2, 1), (0, 0), (1, 2), (0, 0), (1, 3))
        assert len(order) > m.max_batch
        many = r.pool.generate_many([(r.ps[k], r.suffixes[q]) for k, q in order], max_new_tokens=r.T, _return_extras=True)
        rep = m.last_mask_reports()
        assert len(rep) == len(order)
        for i, (k, q) in enumerate(order):
            one = many[i]
            assert len(rep[i]["area"]) == one[2]["nseg"]
            check_entries([rep[i]], None if one[1] is None else [one[1]], [(HH[k], WW[k])], f"{mode} generate_many item {i}")
        assert len(rep[1]["area"]) >= 1 and torch.equal(rep[1]["area"], rep[3]["area"]), "items 1 and 3 ask the rigged question"
    finally:
        m.set_mask_reports(False)
    r.pool.generate_many([(r.ps[0], r.suffixes[0])], max_new_tokens=2)
    with pytest.raises(RuntimeError, match="mask reports are off"):
        m.last_mask_reports()


# ----------------------------------------------------------------------------------------------------------------------
# a packed buffer one word too small
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_packed_buffer_one_word_too_small(mode):
    r = rig(mode, 1)
    m = r.m
    n = len(r.plain["masks"][0])
    need = n * r.H[0] * packed_width(r.W[0])
    buf = torch.full((need + 8,), -77, dtype=torch.int32, device="cuda")
    m.set_mask_reports(True, OFFSET, packed=False)             # (the Python layer arms nothing of its own now)
    try:
        assert m.lib.anyref_set_packed_masks(m.h, ptr(buf), need - 1) == 0
        with pytest.raises(RuntimeError, match=f"cap_words is {need - 1}"):
            r.gen()
        torch.cuda.synchronize()
        assert bool((buf[need - 1:] == -77).all()), "words past the capacity were written"
        left = buf.clone()
        d = gen(r)                                              # nothing stayed armed: the next call runs, without the buffer
        torch.cuda.synchronize()
        assert torch.equal(buf, left), "the refused call's buffer was still armed"
        same_answer(d, r.plain, "the call after the refusal")
        check_entries(d["reports"], d["masks"], r.hw, f"{mode} after the refusal", packed=False)
        # exactly enough is enough
        assert m.lib.anyref_set_packed_masks(m.h, ptr(buf), need) == 0
        d = r.gen()
        po = torch.zeros(1, dtype=torch.long)
        nn, rec = torch.zeros(1, dtype=torch.int32), torch.zeros(1, T_NEW, 8, dtype=torch.int32)
        assert m.lib.anyref_mask_reports(m.h, 1, T_NEW, ptr(nn), ptr(rec), ptr(po)) == 0
        assert int(nn[0]) == n and int(po[0]) == 0
        words = buf[:need].view(n, r.H[0], -1)
        assert np.array_equal(unpack(words, r.W[0]), d["masks"][0].numpy() > 0)
        assert bool((buf[need:] == -77).all())
        assert m.lib.anyref_mask_reports(m.h, 1, max(n - 1, 0), ptr(nn), ptr(rec), ptr(po)) != 0, "a row holds more than seg_cap"
    finally:
        m.set_mask_reports(True, OFFSET, packed=True)
