"""Image sessions (include/anyref_hip.h `anyref_session_open` / `anyref_session_generate`): one image encoded
once, its queries answered behind the cached prefix.

1. a session's Q-row answer against Q plain `generate` calls on prefix + suffix, same handle (parity, parity16);
2. later calls on one session (other suffixes, a larger and a smaller Q) against a fresh session, bit for bit;
3. drafts inside a session; 4. an extra (audio) row in a suffix; 5. refusals and the ways a session is lost;
6. the 16-bit modes, where ids are not pinned: prompt hidden rows against the plain call's, structure of the rest;
7. LLaMA-7B widths (two layers): the tile forms and the broadcast's 16-byte path at the real row size.
Every bound is one the project already uses (tests/test_gpu_e2e.py, tests/test_gpu_draft.py).
"""
import ctypes as C
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from anyref_amd.config import AUDIO_REF_INDEX, IMAGE_TOKEN_INDEX, config_tiny  # noqa: E402
from anyref_amd.synth import synth_state_dict  # noqa: E402
from test_gpu_draft import build, extend_case, same_result  # noqa: E402
from test_gpu_e2e import MASK_TOL, PERF_HIDDEN_REL, PERF_HIDDEN_REL_7B, make_inputs, pad, rig_seg  # noqa: E402

T_NEW = 6
SIZES, HH, WW = [(224, 180)], [300], [241]


class SRig:
    """one handle, one image, a prefix with several ids in front of the placeholder, ragged suffixes (one of length 1)"""

    def __init__(self, mode, cfg=None, sd=None, max_batch=3, n_pre=5, suf_lens=(9, 1, 5, 7, 3), seed=3, rig=True, T=T_NEW, **kw):
        self.cfg = cfg = cfg or config_tiny()
        self.sd = sd if sd is not None else synth_state_dict(cfg, seed=seed, scale=0.05)
        self.T = T
        self.clip, self.sam, _ = make_inputs(cfg, 1, seed=seed + 1)
        g = torch.Generator().manual_seed(seed + 2)
        body = lambda n: torch.randint(3, cfg.llm.vocab - 10, (n,), generator=g)
        self.prefix = torch.cat([torch.tensor([1]), body(n_pre - 1), torch.tensor([IMAGE_TOKEN_INDEX])])
        self.suffixes = [body(n) for n in suf_lens]
        self.P = len(self.prefix) + cfg.clip.n_patches - 1
        if rig:       # the answer to query 0 holds a [SEG]
            rig_seg(cfg, self.sd, self.clip, self.sam, [self.full(0)], SIZES, (HH, WW))
        self.m = build(cfg, self.sd, mode, max_batch=max_batch, max_seg=T, **kw)
        self._plain = {}

    def full(self, q):
        return torch.cat([self.prefix, self.suffixes[q]])

    def open(self):
        return self.m.image_session(self.clip[0], self.sam, SIZES, HH, WW, self.prefix)

    @staticmethod
    def pack(out, ex):
        ids, masks = out[0], out[1]
        return dict(ids=ids.cpu(), lens=ex["out_lens"].tolist(), nseg=ex["nseg"].tolist(),
                    masks=None if masks is None else [t.cpu() for t in masks], hidden=ex["hidden"].cpu(), low=ex["low_res"].cpu(),
                    offered=ex["draft_offered"].tolist(), accepted=ex["draft_accepted"].tolist(), steps=ex["decode_steps"],
                    passes=ex["verify_passes"])

    def plain(self, q, audios=None):
        """the plain call on prefix + suffix q (ends any session); cached"""
        if q not in self._plain:
            out, ex = self.m.generate(self.clip, self.full(q)[None], self.sam, SIZES, HH, WW, max_new_tokens=self.T,
                                      _return_extras=True, audios=audios)
            self._plain[q] = self.pack(out, ex)
        return self._plain[q]

    def ask(self, sess, qs, draft=None, T=None, audios=None, full=False):
        rows = [self.full(q) if full else self.suffixes[q] for q in qs]
        padded, mask = pad(rows)
        out, ex = sess.generate(padded, attention_masks=mask, max_new_tokens=T or self.T, draft_ids=draft, audios=audios,
                                _return_extras=True)
        return self.pack(out, ex)

    def row(self, r, b):
        """row b of a session answer in the shape of a one-row plain answer"""
        n = r["lens"][b]
        masks = None if r["masks"] is None or r["nseg"][b] == 0 else [r["masks"][b]]
        return dict(ids=r["ids"][b: b + 1, :n], masks=masks, hidden=r["hidden"][b: b + 1], low=r["low"][b: b + 1], lens=[n],
                    nseg=[r["nseg"][b]])

    def new(self, r, b, q):
        return r["ids"][b, len(self.full(q)): r["lens"][b]].tolist()

    def check(self, r, qs, what, audios=None):
        """a session answer against the plain calls: ids identical, out_lens / out_nseg equal, masks within MASK_TOL, prompt and
        answer hidden rows within 2e-4 (same_result)"""
        for b, q in enumerate(qs):
            p = self.plain(q, audios=None if audios is None else [audios[b]])
            a = self.row(r, b)
            assert a["lens"] == p["lens"] and a["nseg"] == p["nseg"], f"{what}: row {b} out_lens / out_nseg {a['lens']}, {a['nseg']} vs {p['lens']}, {p['nseg']}"
            rows = self.P + len(self.suffixes[q]) + (p["lens"][0] - len(self.full(q))) - 1
            same_result(a, p, f"{what}: row {b} (query {q})", rows=[rows])


def bitwise(a, b, what, rows):
    """two session answers: ids, masks, low-res logits and the hidden rows that exist, bit for bit"""
    same_result(a, b, what, bitwise=True)
    assert a["lens"] == b["lens"] and a["nseg"] == b["nseg"], what
    for bb, n in enumerate(rows):
        assert torch.equal(a["hidden"][bb, :n], b["hidden"][bb, :n]), f"{what}: hidden rows of row {bb} differ"


@functools.lru_cache(maxsize=None)
def srig(mode):
    r = SRig(mode)
    p0 = r.plain(0)
    assert p0["masks"] is not None and p0["nseg"][0] >= 1, "query 0 was rigged to answer with a [SEG]"
    print(f"[{mode}] plain answers: {[r.new(r.plain(q), 0, q) for q in range(5)]}")
    return r


def hidden_rows(r, qs, res):
    return [r.P + len(r.suffixes[q]) + (res["lens"][b] - len(r.full(q))) - 1 for b, q in enumerate(qs)]


# ----------------------------------------------------------------------------------------------------------------------
# 1. a session against plain generate
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity", "parity16"])
@pytest.mark.parametrize("Q", [1, 2, 3])
def test_session_equals_plain_calls(mode, Q):
    r = srig(mode)
    qs = list(range(Q))
    for q in qs:
        r.plain(q)                      # before the session: a plain call ends it
    with r.open() as sess:
        a = r.ask(sess, qs)
        assert a["passes"] == 0 and a["steps"] == T_NEW - 1 and a["offered"] == [0] * Q
        r.check(a, qs, f"{mode} Q={Q}")
        # hidden rows [0, P) of every query are the prefix's: rows 1.. were filled by the broadcast, bit for bit
        for b in range(1, Q):
            assert torch.equal(a["hidden"][b, : r.P], a["hidden"][0, : r.P])
        # full prompts, as a data loader produces them, are cut at the placeholder: the same call
        f = r.ask(sess, qs, full=True)
        bitwise(f, a, "full prompts", hidden_rows(r, qs, a))
        assert f["ids"][0, : len(r.prefix)].tolist() == r.prefix.tolist(), "output rows start with the prefix"


# ----------------------------------------------------------------------------------------------------------------------
# 2. later calls on the same session
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity", "parity16"])
def test_later_calls_equal_a_fresh_session(mode):
    r = srig(mode)
    for q in range(5):
        r.plain(q)
    with r.open() as sess:
        first = r.ask(sess, [0])                 # Q = 1: nothing is broadcast
        a3 = r.ask(sess, [0, 1, 2])              # larger: rows 1, 2 receive the prefix
        b2 = r.ask(sess, [3, 4])                 # smaller, other suffixes: nothing is broadcast, rows 0, 1 still hold it
        c3 = r.ask(sess, [4, 2, 3])              # the same three rows again
    with r.open() as sess:
        a3f = r.ask(sess, [0, 1, 2])
    with r.open() as sess:
        b2f = r.ask(sess, [3, 4])
    with r.open() as sess:
        c3f = r.ask(sess, [4, 2, 3])
    bitwise(a3, a3f, "Q = 3 after Q = 1", hidden_rows(r, [0, 1, 2], a3))
    bitwise(b2, b2f, "Q = 2 after Q = 3", hidden_rows(r, [3, 4], b2))
    bitwise(c3, c3f, "Q = 3 again", hidden_rows(r, [4, 2, 3], c3))
    r.check(first, [0], "first")
    r.check(b2, [3, 4], "Q = 2 after Q = 3")     # ... and both still are what the plain calls give
    r.check(c3, [4, 2, 3], "Q = 3 again")
    for b in range(2):
        assert torch.equal(b2["hidden"][b, : r.P], a3["hidden"][0, : r.P]), "rows 0 and 1 still hold the prefix"


# ----------------------------------------------------------------------------------------------------------------------
# 3. drafts inside a session
# ----------------------------------------------------------------------------------------------------------------------
def test_drafts_inside_a_session():
    r = srig("parity")
    qs = [0, 1]
    true = [r.new(r.plain(q), 0, q)[:5] for q in qs]
    with r.open() as sess:
        p = r.ask(sess, qs)
        d = r.ask(sess, qs, draft=true)
        assert d["offered"] == [5, 5] and d["accepted"] == [5, 5] and d["steps"] == 0 and d["passes"] == 1, d
        r.check(d, qs, "true draft")
        same_result(d, p, "true draft vs no draft", rows=hidden_rows(r, qs, p))
        wrong = [list(t) for t in true]
        wrong[0][2] = (wrong[0][2] + 1) % r.cfg.llm.vocab
        w = r.ask(sess, qs, draft=wrong)
        assert w["offered"] == [5, 5] and w["accepted"] == [2, 5] and w["steps"] == 3 and w["passes"] == 1, w
        r.check(w, qs, "draft wrong at 2")
        # one-shot: the next call has none
        n = r.ask(sess, qs)
        assert n["offered"] == [0, 0] and n["passes"] == 0 and n["steps"] == T_NEW - 1
        bitwise(n, p, "no stale draft", hidden_rows(r, qs, p))
        # a draft armed for another batch size is refused and consumed
        r.m.set_draft([true[0]])
        with pytest.raises(RuntimeError, match="batch size"):
            r.ask(sess, qs)
        assert r.ask(sess, qs)["offered"] == [0, 0]
        # "last" is a policy of model.generate: not applied here
        r.m.set_draft_policy("last")
        try:
            assert r.ask(sess, qs)["offered"] == [0, 0] and r.ask(sess, qs)["offered"] == [0, 0]
        finally:
            r.m.set_draft_policy(None)


# ----------------------------------------------------------------------------------------------------------------------
# 4. an extra row in a suffix
# ----------------------------------------------------------------------------------------------------------------------
def test_extra_row_in_a_suffix():
    r = SRig("parity", max_batch=2, seed=5, rig=False)
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(1, r.cfg.audio_dim, generator=g)
    s1 = r.suffixes[1] = torch.cat([r.suffixes[3][:2], torch.tensor([AUDIO_REF_INDEX]), r.suffixes[3][2:]])
    assert int(s1[2]) == AUDIO_REF_INDEX
    aud = [None, emb]
    r.plain(0)
    r.plain(1, audios=[emb])
    with r.open() as sess:
        a = r.ask(sess, [0, 1], audios=aud)
        r.check(a, [0, 1], "audio row", audios=aud)
        with pytest.raises(RuntimeError, match="extra row"):          # a placeholder nobody provides a row for
            r.ask(sess, [0, 1])
        r.check(r.ask(sess, [0, 1], audios=aud), [0, 1], "after the refusal", audios=aud)


# ----------------------------------------------------------------------------------------------------------------------
# 5. refusals and loss
# ----------------------------------------------------------------------------------------------------------------------
def raw_generate(m, suffix, T):
    """anyref_session_generate itself on one suffix (what the Python layer would never pass)"""
    suf = torch.tensor([suffix], dtype=torch.long)
    ln = torch.tensor([len(suffix)], dtype=torch.int32)
    out_ids = torch.zeros(1, 64 + len(suffix) + T, dtype=torch.long)
    i32 = lambda: torch.zeros(1, dtype=torch.int32)
    out_lens, nseg, offs = i32(), i32(), torch.zeros(1, dtype=torch.long)
    cap = m.max_seg * HH[0] * WW[0]
    masks = torch.empty(cap, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = m.lib.anyref_session_generate(m.h, m._stream(), ptr(suf), ptr(ln), 1, len(suffix), None, None, 0, T, -1, ptr(out_ids),
                                       ptr(out_lens), ptr(nseg), ptr(masks), cap, ptr(offs), None, None)
    return rc, m.lib.anyref_last_error(m.h).decode()


def test_refusals_leave_the_session_usable():
    r = srig("parity")
    qs = [0, 1]
    for q in qs:
        r.plain(q)
    S = r.cfg.llm.max_seq
    with r.open() as sess:
        want = r.ask(sess, qs)
        r.check(want, qs, "before")

        def still_fine(what):
            bitwise(r.ask(sess, qs), want, f"after {what}", hidden_rows(r, qs, want))

        # P + lens + max_new_tokens past the cache: query 0 has 9 ids
        with pytest.raises(RuntimeError, match="llm_max_seq"):
            r.ask(sess, qs, T=S - r.P - 9 + 1)
        still_fine("llm_max_seq")
        # an image placeholder inside a suffix: the host rule names the row, the C entry refuses what gets past it
        with pytest.raises(ValueError, match="row 1 does not begin"):
            bad, bad_mask = pad([r.suffixes[0], torch.cat([r.suffixes[1], torch.tensor([IMAGE_TOKEN_INDEX, 5])])])
            sess.generate(bad, attention_masks=bad_mask, max_new_tokens=2)
        rc, msg = raw_generate(r.m, [5, IMAGE_TOKEN_INDEX, 6], 2)
        assert rc != 0 and "placeholder" in msg, msg
        rc, msg = raw_generate(r.m, [5, 6], 0)
        assert rc != 0 and "max_new_tokens" in msg, msg
        still_fine("placeholder")
        # more queries than max_batch
        with pytest.raises((ValueError, RuntimeError), match="max_batch"):
            r.ask(sess, [0, 1, 2, 3])
        still_fine("max_batch")
    # lost: an intervening generate, llm_forward; re-opening works
    sess = r.open()
    r.m.generate(r.clip, r.full(0)[None], r.sam, SIZES, HH, WW, max_new_tokens=2)
    with pytest.raises(RuntimeError, match="session lost: ended by anyref_generate"):
        r.ask(sess, qs)
    sess = r.open()
    r.m.llm_forward(torch.zeros(1, 4, r.cfg.llm.dim))
    with pytest.raises(RuntimeError, match="session lost: ended by anyref_llm_forward"):
        r.ask(sess, qs)
    with r.open() as sess:
        bitwise(r.ask(sess, qs), want, "re-opened", hidden_rows(r, qs, want))
    # no session open: a closed one, in Python and at the C entry
    with pytest.raises(RuntimeError, match="session"):
        r.ask(sess, qs)
    rc, msg = raw_generate(r.m, [5, 6], 2)
    assert rc != 0 and "no session open" in msg, msg
    # a prefix that does not end with its only placeholder never reaches the backend
    with pytest.raises(ValueError, match="placeholder"):
        r.m.image_session(r.clip[0], r.sam, SIZES, HH, WW, r.prefix[:-1])


def test_rephrase_is_refused_inside_a_session():
    cfg = config_tiny()
    cfg.rephrase_weight = 0.5
    r = SRig("parity", cfg=cfg, max_batch=1, seed=7, rig=False)
    with r.open() as sess:
        with pytest.raises(RuntimeError, match="rephrase_weight > 0"):
            r.ask(sess, [0])


# ----------------------------------------------------------------------------------------------------------------------
# 6. 16-bit modes: ids are not pinned
# ----------------------------------------------------------------------------------------------------------------------
def prompt_rows_error(r, qs):
    """max |hidden(session) - hidden(plain)| over the prefix and suffix rows (they do not depend on generated ids), and its scale;
    plus the session answer"""
    for q in qs:
        r.plain(q)
    with r.open() as sess:
        a = r.ask(sess, qs)
    err = scale = 0.0
    for b, q in enumerate(qs):
        n = r.P + len(r.suffixes[q])
        ref = r.plain(q)["hidden"][0, :n]
        err = max(err, (a["hidden"][b, :n] - ref).abs().max().item())
        scale = max(scale, ref.abs().max().item())
    return err, scale, a


@functools.lru_cache(maxsize=None)
def perf_error_tiny():
    return prompt_rows_error(SRig("perf"), [0, 1, 2])[:2]


@pytest.mark.parametrize("mode", ["perf", "perf_f16", "perf_int4w", "perf_fp8w"])
def test_16_bit_modes(mode):
    """perf_int4w is bounded as its own tests bound it: twice perf's error on the same rows, measured here"""
    qs = [0, 1, 2]
    r = SRig(mode)
    err, scale, a = prompt_rows_error(r, qs)
    bound = PERF_HIDDEN_REL * scale
    if mode == "perf_int4w":
        pe, ps = perf_error_tiny()
        bound = 2 * pe
        print(f"[perf] session vs plain prompt hidden err {pe:.3e} (scale {ps:.2f}) -> int4w bound {bound:.3e}")
    print(f"[{mode}] session vs plain prompt hidden err {err:.3e} (scale {scale:.2f}, bound {bound:.3e}); "
          f"answers {[r.new(a, b, q) for b, q in enumerate(qs)]}, nseg {a['nseg']}")
    assert err <= bound, (err, bound)
    structure(r, a, qs)


def structure(r, a, qs):
    for b, q in enumerate(qs):
        assert a["lens"][b] == len(r.full(q)) + r.T, "no EOS id: every row holds max_new_tokens new tokens"
        assert a["ids"][b, : len(r.full(q))].tolist() == r.full(q).tolist()
        assert 0 <= a["nseg"][b] <= r.T
        n = r.P + len(r.suffixes[q]) + r.T - 1
        assert torch.isfinite(a["hidden"][b, :n]).all()
    assert (a["masks"] is None) == (sum(a["nseg"]) == 0)
    for b, t in enumerate(a["masks"] or []):
        assert t.shape == (a["nseg"][b], HH[0], WW[0]) and torch.isfinite(t).all()


# ----------------------------------------------------------------------------------------------------------------------
# 7. LLaMA-7B widths
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["perf", "parity16"])
def test_llama_7b_widths(mode):
    """dim 4096, 32 heads, mlp 11008, two layers, max_seq 512; prefix 45 ids (44 and the placeholder: 300 spliced rows), suffixes of 9, Q = 2"""
    cfg, sd = extend_case(1)[:2]
    cfg = dataclasses.replace(cfg)          # (the cached case is shared with tests/test_gpu_draft.py: the [SEG] id is set on a copy)
    T = 4
    r = SRig(mode, cfg=cfg, sd=sd, max_batch=2, n_pre=44, suf_lens=(9, 9), seed=41, rig=False, T=T)
    assert r.P == 300
    qs = [0, 1]
    # name the third token of query 0's answer [SEG]: masks on both paths
    r.m.set_seg_token_idx(int(r.new(r.plain(0), 0, 0)[2]))
    r._plain.clear()
    if mode == "parity16":
        for q in qs:
            r.plain(q)
        assert r.plain(0)["nseg"][0] >= 1
        with r.open() as sess:
            a = r.ask(sess, qs)
        r.check(a, qs, "7B widths")
        return
    err, scale, a = prompt_rows_error(r, qs)
    bound = PERF_HIDDEN_REL_7B * scale
    print(f"[{mode}, 7B widths] session vs plain prompt hidden err {err:.3e} (scale {scale:.2f}, bound {bound:.3e}); nseg {a['nseg']}")
    assert err <= bound, (err, bound)
    structure(r, a, qs)
