"""Session pools (include/anyref_hip.h `anyref_session_pool_reserve` / `_store` / `_generate_pooled`): several
images resident in slots, queries about different images in one call.

1. a pooled call whose rows all name one slot against `anyref_session_generate` on a live session of that image, bit for bit;
2. mixed rows against the homogeneous calls with the same Q and lens, row by row, bit for bit; 3. pooled rows against plain
`generate` on prefix + suffix, within the bounds tests/test_gpu_session.py uses for a session; 4. slots survive the calls that end
a session, and an unchanged assignment skips its gathers; 5. loss, refusals, closing, replacing; 6. drafts and rephrasing in mixed
calls; 7. the 16-bit modes; 8. LLaMA-7B widths at two layers; 9. the Python pool: eviction and `generate_many`.
Every bound is one the project already uses (tests/test_gpu_session.py, tests/test_gpu_e2e.py, tests/test_gpu_draft.py).
"""
import ctypes as C
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from anyref_amd.config import IMAGE_TOKEN_INDEX, config_tiny  # noqa: E402
from anyref_amd.synth import synth_state_dict  # noqa: E402
from test_gpu_draft import build, extend_case, same_result  # noqa: E402
from test_gpu_e2e import MASK_TOL, PERF_HIDDEN_REL, PERF_HIDDEN_REL_7B, make_inputs, pad, rig_seg  # noqa: E402
from test_gpu_session import SRig, bitwise  # noqa: E402

T_NEW = 6
SIZES, HH, WW = [(224, 180), (200, 224), (224, 224)], [300, 211, 224], [241, 280, 224]
QS = [0, 1, 2]


class PRig:
    """one handle, K images with prefixes of two lengths (image 1's is longer), ragged suffixes shared by the images, every image
    stored in its own slot of a pool"""

    def __init__(self, mode, cfg=None, sd=None, max_batch=3, K=3, n_pre=(5, 8, 5), suf_lens=(9, 1, 5, 7), seed=3, rig=True, T=T_NEW,
                 slots=None, **kw):
        self.cfg = cfg = cfg or config_tiny()
        self.sd = sd if sd is not None else synth_state_dict(cfg, seed=seed, scale=0.05)
        self.T, self.K = T, K
        self.clip, self.sam, _ = make_inputs(cfg, K, seed=seed + 1)
        g = torch.Generator().manual_seed(seed + 2)
        body = lambda n: torch.randint(3, cfg.llm.vocab - 10, (n,), generator=g)
        self.prefix = [torch.cat([torch.tensor([1]), body(n - 1), torch.tensor([IMAGE_TOKEN_INDEX])]) for n in n_pre[:K]]
        self.suffixes = [body(n) for n in suf_lens]
        self.P = [len(p) + cfg.clip.n_patches - 1 for p in self.prefix]
        if rig:       # image 0's answer to query 0 holds a [SEG]
            rig_seg(cfg, self.sd, self.clip, self.sam, [self.full(0, 0)], SIZES, (HH, WW))
        self.m = build(cfg, self.sd, mode, max_batch=max_batch, max_seg=T, **kw)
        self.pool = self.m.session_pool(slots or K)
        self.ps = [self.open(k, k) for k in range(K)]
        self._plain = {}

    def open(self, key, k):
        return self.pool.open(key, self.clip[k], self.sam[k], SIZES[k], HH[k], WW[k], self.prefix[k])

    def live(self, k):
        return self.m.image_session(self.clip[k], self.sam[k], SIZES[k], HH[k], WW[k], self.prefix[k])

    def full(self, k, q):
        return torch.cat([self.prefix[k], self.suffixes[q]])

    def plain(self, k, q):
        if (k, q) not in self._plain:
            out, ex = self.m.generate(self.clip[k: k + 1], self.full(k, q)[None], self.sam[k: k + 1], [SIZES[k]], [HH[k]], [WW[k]],
                                      max_new_tokens=self.T, _return_extras=True)
            self._plain[k, q] = SRig.pack(out, ex)
        return self._plain[k, q]

    def pooled(self, ks, qs=QS, draft=None, full=False, sessions=None):
        rows = [self.full(k, q) if full else self.suffixes[q] for k, q in zip(ks, qs)]
        padded, mask = pad(rows)
        out, ex = self.pool.generate(sessions or [self.ps[k] for k in ks], padded, attention_masks=mask, max_new_tokens=self.T,
                                     draft_ids=draft, _return_extras=True)
        return SRig.pack(out, ex)

    def single(self, k, qs=QS):
        """anyref_session_generate on a live session of image k"""
        padded, mask = pad([self.suffixes[q] for q in qs])
        with self.live(k) as sess:
            out, ex = sess.generate(padded, attention_masks=mask, max_new_tokens=self.T, _return_extras=True)
        return SRig.pack(out, ex)

    def rows(self, r, ks, qs=QS):
        """hidden rows that exist per row of an answer"""
        return [self.P[k] + len(self.suffixes[q]) + (r["lens"][b] - len(self.full(k, q))) - 1 for b, (k, q) in enumerate(zip(ks, qs))]

    def new(self, r, b, k, q):
        return r["ids"][b, len(self.full(k, q)): r["lens"][b]].tolist()

    @functools.lru_cache(maxsize=None)
    def hom(self, k):
        """the pooled call whose rows all name slot k, queries QS (cached: a reference the tests share and leave unchanged)"""
        return self.pooled([k] * len(QS))

    def rows_equal_hom(self, r, ks, what):
        """row b of r against row b of the homogeneous call of its slot, bit for bit"""
        for b, k in enumerate(ks):
            h = self.hom(k)
            n = self.rows(h, [k] * len(QS))[b]
            bitwise(SRig.row(None, r, b), SRig.row(None, h, b), f"{what}: row {b} (slot {k})", [n])

    def against_plain(self, r, ks, what, qs=QS):
        """test_session_equals_plain_calls' check (SRig.check) per pooled row: ids identical, out_lens / out_nseg equal, masks
        within MASK_TOL, prompt and answer hidden rows within 2e-4"""
        for b, (k, q) in enumerate(zip(ks, qs)):
            p, a = self.plain(k, q), SRig.row(None, r, b)
            assert a["lens"] == p["lens"] and a["nseg"] == p["nseg"], f"{what}: row {b} {a['lens']}, {a['nseg']} vs {p['lens']}, {p['nseg']}"
            n = self.P[k] + len(self.suffixes[q]) + (p["lens"][0] - len(self.full(k, q))) - 1
            same_result(a, p, f"{what}: row {b} (image {k}, query {q})", rows=[n])


@functools.lru_cache(maxsize=None)
def prig(mode):
    return PRig(mode)


# ----------------------------------------------------------------------------------------------------------------------
# 1 - 3. pooled = single session; mixed rows = homogeneous rows; pooled rows against plain calls
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity", "parity16"])
def test_pooled_equals_single_session(mode):
    r = prig(mode)
    assert r.P[0] == r.P[2] != r.P[1], "two prefix lengths"
    for k in range(3):
        h = r.hom(k)
        bitwise(h, r.single(k), f"{mode}: slot {k} against a live session", r.rows(h, [k] * 3))
        assert h["ids"][0, : len(r.prefix[k])].tolist() == r.prefix[k].tolist(), "output rows start with the slot's prefix"
    assert r.hom(0)["masks"] is not None and r.hom(0)["nseg"][0] >= 1, "image 0, query 0 was rigged to answer with a [SEG]"


@pytest.mark.parametrize("mode", ["parity", "parity16"])
@pytest.mark.parametrize("ks", [(0, 1, 2), (1, 1, 0)])
def test_mixed_rows_equal_homogeneous_rows(mode, ks):
    r = prig(mode)
    a = r.pooled(ks)
    r.rows_equal_hom(a, ks, f"{mode} {ks}")
    f = r.pooled(ks, full=True)                       # full prompts, each cut against its own session's prefix
    bitwise(f, a, "full prompts", r.rows(a, ks))
    with pytest.raises(ValueError, match="row 1 does not begin"):
        r.pooled(ks, full=True, sessions=[r.ps[ks[0]], r.ps[0], r.ps[ks[2]]])     # row 1 is about image 1, session 0 given


@pytest.mark.parametrize("mode", ["parity", "parity16"])
def test_pooled_rows_against_plain_calls(mode):
    r = prig(mode)
    for ks in ((0, 1, 2), (1, 1, 0), (2, 2, 2)):
        for k, q in zip(ks, QS):
            r.plain(k, q)
        r.against_plain(r.pooled(ks), ks, f"{mode} {ks}")
    r.against_plain(r.pooled((1,), qs=[3]), (1,), "Q = 1", qs=[3])


# ----------------------------------------------------------------------------------------------------------------------
# 4. survival
# ----------------------------------------------------------------------------------------------------------------------
def test_slots_survive_what_ends_a_session():
    r = prig("parity")
    ks = (0, 1, 2)
    before = r.pooled(ks)
    rows = r.rows(before, ks)
    m, full = r.m, r.full(0, 0)
    enders = [lambda: m.generate(r.clip[:1], full[None], r.sam[:1], SIZES[:1], HH[:1], WW[:1], max_new_tokens=2),
              lambda: m.model_forward_new(r.clip[:1], r.sam[:1], full[None], full[None].clone(), None, SIZES[:1], None, HH[:1], WW[:1]),
              lambda: m.llm_forward(torch.zeros(3, 4, r.cfg.llm.dim)),
              lambda: m.encode_images(r.clip)]
    for i, end in enumerate(enders):
        sess = r.live(1)
        end()
        with pytest.raises(RuntimeError, match="session lost: ended by anyref_"):
            sess.generate(r.suffixes[0][None], max_new_tokens=2)
        after = r.pooled(ks)
        bitwise(after, before, f"after ender {i}", rows)
        st = r.pool.stats()
        assert (st["rows_gathered"], st["rows_skipped"]) == (3, 0) and st["gather_ms"] is not None and st["gather_ms"] > 0, st
        again = r.pooled(ks)
        st = r.pool.stats()
        assert (st["rows_gathered"], st["rows_skipped"]) == (0, 3) and st["gather_ms"] is None, st
        bitwise(again, before, f"all rows skipped after ender {i}", rows)
    # a pooled call ends the unpooled session itself, and says so
    sess = r.live(2)
    r.pooled(ks)
    with pytest.raises(RuntimeError, match="session lost: ended by anyref_session_generate_pooled"):
        sess.generate(r.suffixes[0][None], max_new_tokens=2)
    st = r.pool.stats()
    assert st["slots"] == 3 and st["in_use"] == 3 and st["bytes"] > 0
    assert st["bytes"] <= m.device_bytes


# ----------------------------------------------------------------------------------------------------------------------
# 5. loss and refusal
# ----------------------------------------------------------------------------------------------------------------------
def raw_pooled(m, slots, suffixes, T, lens=None):
    """anyref_session_generate_pooled itself (what the Python layer would never pass)"""
    Q, Lmax = len(suffixes), max([len(s) for s in suffixes] + [1])
    suf = torch.zeros(max(Q, 1), Lmax, dtype=torch.long)
    for b, s in enumerate(suffixes):
        suf[b, : len(s)] = torch.tensor(s, dtype=torch.long)
    ln = torch.tensor((lens or [len(s) for s in suffixes]) + [0], dtype=torch.int32)      # (one spare entry: Q = 0 passes
    sl = torch.tensor(list(slots) + [0], dtype=torch.int32)                               #  no null pointers)
    out_ids = torch.zeros(max(Q, 1), 64 + Lmax + max(T, 0), dtype=torch.long)
    i32 = lambda: torch.zeros(max(Q, 1), dtype=torch.int32)
    out_lens, nseg, offs = i32(), i32(), torch.zeros(max(Q, 1), dtype=torch.long)
    cap = max(Q, 1) * m.max_seg * max(HH) * max(WW)
    masks = torch.empty(cap, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = m.lib.anyref_session_generate_pooled(m.h, m._stream(), ptr(sl), ptr(suf), ptr(ln), Q, Lmax, None, None, 0, T, -1,
                                              ptr(out_ids), ptr(out_lens), ptr(nseg), ptr(masks), cap, ptr(offs), None, None)
    return rc, m.lib.anyref_last_error(m.h).decode()


def test_refusals_leave_pool_and_session_usable():
    r = PRig("parity", slots=4)
    m, ks = r.m, (0, 1, 2)
    want = r.pooled(ks)
    rows = r.rows(want, ks)
    S, V = r.cfg.llm.max_seq, r.cfg.llm.vocab
    sess = r.live(1)                                   # a live session beside the pool: refusals leave it usable too
    live_want = SRig.pack(*sess.generate(r.suffixes[0][None], max_new_tokens=r.T, _return_extras=True))
    for slots, sufs, T, lens, what in (
            ([3], [[5, 6]], 2, None, "slot 3 is empty"),
            ([4], [[5, 6]], 2, None, "slot 4 outside the pool"),
            ([-1], [[5, 6]], 2, None, "outside the pool"),
            ([0, 1, 2, 0], [[5, 6]] * 4, 2, None, "max_batch"),
            ([], [], 2, None, "max_batch"),                                    # Q = 0
            ([1], [[5, 6]], S - r.P[1] - 2 + 1, None, "llm_max_seq"),          # fits slot 0's shorter prefix, not slot 1's
            ([0], [[5, IMAGE_TOKEN_INDEX, 6]], 2, None, "placeholder"),
            ([0], [[5, V + 1]], 2, None, "extra row"),
            ([0], [[5, 6]], 2, [0], "suffix length"),
            ([0], [[5, 6]], 0, None, "max_new_tokens")):
        rc, msg = raw_pooled(m, slots, sufs, T, lens)
        assert rc != 0 and what in msg, (what, msg)
    r.m.set_draft([[1, 2]])
    with pytest.raises(RuntimeError, match="batch size"):
        r.pooled(ks)
    with pytest.raises((ValueError, RuntimeError), match="max_batch"):
        r.pooled((0, 1, 2, 0), qs=[0, 1, 2, 3])
    bitwise(SRig.pack(*sess.generate(r.suffixes[0][None], max_new_tokens=r.T, _return_extras=True)), live_want,
            "the live session after the refused pooled calls", [r.P[1] + 9 + r.T - 1])
    bitwise(r.pooled(ks), want, "after the refusals", rows)
    # store: refused without a live session, outside the pool, past max_prefix_rows
    sess.close()
    assert m.lib.anyref_session_store(m.h, m._stream(), 3) != 0 and b"no session open" in m.lib.anyref_last_error(m.h)
    with r.live(1):
        assert m.lib.anyref_session_store(m.h, m._stream(), 4) != 0 and b"outside the pool" in m.lib.anyref_last_error(m.h)
        assert m.lib.anyref_session_pool_reserve(m.h, 4, r.P[1] - 1) != 0 and b"every slot is empty" in m.lib.anyref_last_error(m.h)
    bitwise(r.pooled(ks), want, "after the refused stores", rows)
    # close and reuse a slot; store replacing a slot
    old = r.ps[2]
    r.pool.close(2)
    with pytest.raises(RuntimeError, match="gone from slot 2"):
        r.pooled(ks)
    rc, msg = raw_pooled(m, [2], [[5, 6]], 2)
    assert rc != 0 and "slot 2 is empty" in msg
    assert r.pool.get(2) is None and r.pool.stats()["in_use"] == 2
    r.ps[2] = r.open("two again", 2)
    assert r.ps[2].slot == 2 and r.ps[2].gen != old.gen and r.pool.get("two again") is r.ps[2]
    bitwise(r.pooled(ks), want, "slot 2 closed and reused", rows)
    h1 = r.pooled((1, 1, 1))
    r.ps[0] = r.open(0, 1)                             # key 0 opened again, now with image 1: same slot, replaced
    assert r.ps[0].slot == 0
    bitwise(r.pooled((0, 0, 0)), h1, "slot 0 replaced by image 1", r.rows(h1, (1, 1, 1)))


def test_what_changes_the_weights_ends_every_slot():
    """anyref_update_weight and anyref_adapter_apply on a handle that reserved its adapter targets; the same weights each time, so
    a re-opened pool answers as before"""
    r = PRig("parity", K=2, max_batch=2, rig=False, adapters="qv")
    m, ks, qs = r.m, (0, 1), [0, 1]
    a = r.pooled(ks, qs)
    rows = r.rows(a, ks, qs)
    m._update_weight("lm_head.weight", r.sd["lm_head.weight"])
    rc, msg = raw_pooled(m, [1], [[5, 6]], 2)
    assert rc != 0 and "slot 1 lost: ended by anyref_update_weight" in msg, msg
    with pytest.raises(RuntimeError, match="gone from slot"):      # the Python pool was told: its sessions are stale
        r.pooled(ks, qs)
    assert r.pool.stats()["in_use"] == 0 and r.pool.get(0) is None and r.pool.get(1) is None and len(r.pool.table) == 0
    r.ps = [r.open(k, k) for k in range(2)]
    bitwise(r.pooled(ks, qs), a, "re-opened after update_weight", rows)
    m.set_adapter(None)
    rc, msg = raw_pooled(m, [0], [[5, 6]], 2)
    assert rc != 0 and "slot 0 lost: ended by anyref_adapter_apply" in msg, msg
    with pytest.raises(RuntimeError, match="gone from slot"):
        r.pooled(ks, qs)
    assert r.pool.get(0) is None and r.pool.stats()["in_use"] == 0
    r.ps = [r.open(k, k) for k in range(2)]
    bitwise(r.pooled(ks, qs), a, "the base again", rows)


# ----------------------------------------------------------------------------------------------------------------------
# 6. drafts and rephrasing
# ----------------------------------------------------------------------------------------------------------------------
def test_drafts_in_a_mixed_call():
    r = prig("parity")
    ks, qs = (1, 0), [0, 1]
    p = r.pooled(ks, qs)
    true = [r.new(p, b, k, q)[:5] for b, (k, q) in enumerate(zip(ks, qs))]
    wrong = [list(true[0]), list(true[1])]
    wrong[1][2] = (wrong[1][2] + 1) % r.cfg.llm.vocab
    d = r.pooled(ks, qs, draft=wrong)
    assert d["offered"] == [5, 5] and d["accepted"] == [5, 2] and d["passes"] == 1, d
    same_result(d, p, "one draft accepted, one corrupted", rows=r.rows(p, ks, qs))
    assert d["lens"] == p["lens"] and d["nseg"] == p["nseg"]
    n = r.pooled(ks, qs)
    assert n["offered"] == [0, 0] and n["passes"] == 0
    bitwise(n, p, "no stale draft", r.rows(p, ks, qs))


@functools.lru_cache(maxsize=None)
def reph_rig():
    cfg = config_tiny()
    cfg.rephrase_weight = 0.5
    r = PRig("parity", cfg=cfg, seed=3)
    r.m.set_rephrase_paths(True)
    return r


def test_rephrase_in_a_mixed_call():
    r = reph_rig()
    for ks in ((0, 1, 2), (1, 1, 0)):
        r.rows_equal_hom(r.pooled(ks), ks, f"rephrase {ks}")
    assert sum(sum(r.hom(k)["nseg"]) for k in range(3)) >= 1, "some row answers with a [SEG]"
    r.m.set_rephrase_paths(False)
    try:
        with pytest.raises(RuntimeError, match="rephrase_weight > 0"):
            r.pooled((0, 1, 2))
    finally:
        r.m.set_rephrase_paths(True)
    r.rows_equal_hom(r.pooled((0, 1, 2)), (0, 1, 2), "after the refusal")


# ----------------------------------------------------------------------------------------------------------------------
# 7. 16-bit modes
# ----------------------------------------------------------------------------------------------------------------------
def prompt_rows_error(r, a, ks, qs=QS):
    """test_gpu_session.prompt_rows_error for pooled rows: max |hidden(pooled) - hidden(plain)| over the prefix and suffix rows"""
    err = scale = 0.0
    for b, (k, q) in enumerate(zip(ks, qs)):
        n = r.P[k] + len(r.suffixes[q])
        ref = r.plain(k, q)["hidden"][0, :n]
        err = max(err, (a["hidden"][b, :n] - ref).abs().max().item())
        scale = max(scale, ref.abs().max().item())
    return err, scale


@functools.lru_cache(maxsize=None)
def perf_error_tiny():
    """perf's own error on the rows test_16_bit_modes compares: the larger of its two assignments"""
    r = prig("perf")
    return max(prompt_rows_error(r, r.pooled(ks), ks)[0] for ks in ((0, 1, 2), (1, 1, 0)))


@pytest.mark.parametrize("mode", ["perf", "perf_int4w"])
def test_16_bit_modes(mode):
    """tests 1 and 2 bit for bit; test 3 with test_gpu_session.test_16_bit_modes' bounds (perf_int4w: twice perf's error on the
    same rows, measured here)"""
    r = prig(mode)
    for k in range(3):
        bitwise(r.hom(k), r.single(k), f"{mode}: slot {k} against a live session", r.rows(r.hom(k), [k] * 3))
    for ks in ((0, 1, 2), (1, 1, 0)):
        a = r.pooled(ks)
        r.rows_equal_hom(a, ks, f"{mode} {ks}")
        err, scale = prompt_rows_error(r, a, ks)
        bound = PERF_HIDDEN_REL * scale
        if mode == "perf_int4w":
            bound = 2 * perf_error_tiny()
        print(f"[{mode}] {ks} pooled vs plain prompt hidden err {err:.3e} (scale {scale:.2f}, bound {bound:.3e})")
        assert err <= bound, (err, bound)
        for b, (k, q) in enumerate(zip(ks, QS)):
            assert a["lens"][b] == len(r.full(k, q)) + r.T and a["ids"][b, : len(r.full(k, q))].tolist() == r.full(k, q).tolist()


# ----------------------------------------------------------------------------------------------------------------------
# 8. LLaMA-7B widths
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["perf", "parity16"])
def test_llama_7b_widths(mode):
    """dim 4096, 32 heads, mlp 11008, two layers, max_seq 512; two slots with prefixes of 300 and 296 rows, a mixed two-row call"""
    cfg, sd = extend_case(1)[:2]
    cfg = dataclasses.replace(cfg)
    qs = [0, 1]
    r = PRig(mode, cfg=cfg, sd=sd, max_batch=2, K=2, n_pre=(44, 40), suf_lens=(9, 9), seed=41, rig=False, T=4)
    assert r.P == [300, 296]
    hom = [r.pooled((k, k), qs) for k in range(2)]
    for ks in ((0, 1), (1, 0)):
        a = r.pooled(ks, qs)
        for b, k in enumerate(ks):
            n = r.rows(hom[k], (k, k), qs)[b]
            bitwise(SRig.row(None, a, b), SRig.row(None, hom[k], b), f"{mode} 7B widths {ks}: row {b}", [n])
    if mode == "parity16":
        r.against_plain(r.pooled((0, 1), qs), (0, 1), "7B widths", qs=qs)
    else:
        a = r.pooled((0, 1), qs)
        err, scale = prompt_rows_error(r, a, (0, 1), qs)
        print(f"[{mode}, 7B widths] pooled vs plain prompt hidden err {err:.3e} (scale {scale:.2f}, bound {PERF_HIDDEN_REL_7B * scale:.3e})")
        assert err <= PERF_HIDDEN_REL_7B * scale


# ----------------------------------------------------------------------------------------------------------------------
# 9. the Python pool
# ----------------------------------------------------------------------------------------------------------------------
def test_eviction_and_generate_many():
    r = PRig("parity", slots=3)
    items = [(r.ps[k], r.suffixes[q]) for k, q in ((0, 0), (1, 1), (2, 2), (0, 3), (2, 0), (1, 2), (0, 1))]
    singles = [r.pool.generate([ps], ids[None], max_new_tokens=r.T, _return_extras=True) for ps, ids in items]
    many = r.pool.generate_many(items, max_new_tokens=r.T, _return_extras=True)
    assert len(many) == 7
    for i, ((res, ex), got) in enumerate(zip(singles, many)):
        n = int(ex["out_lens"][0])
        assert torch.equal(got[0].cpu(), res[0][0, :n].cpu()), f"item {i}: ids of the 3-row calls and of the single call differ"
        assert got[2]["nseg"] == int(ex["nseg"][0])
        if got[2]["nseg"]:
            assert got[1].shape == res[1][0].shape and (got[1] - res[1][0]).abs().max().item() <= MASK_TOL
        else:
            assert got[1] is None
    st = r.pool.stats()
    assert (st["rows_gathered"], st["rows_skipped"]) == (0, 1), "the last call's one item went into the row that held its image"
    # full pool: a fourth key evicts the least recently used -- key 2 (the last use of 0 and 1 is later)
    r.pool.get(1)
    four = r.open("four", 1)
    assert four.slot == r.ps[2].slot and r.pool.get(2) is None and r.pool.get("four") is four
    with pytest.raises(RuntimeError, match="gone from slot"):
        r.pool.generate([r.ps[2]], r.suffixes[0][None], max_new_tokens=2)
    a = SRig.pack(*r.pool.generate([four], r.suffixes[0][None], max_new_tokens=r.T, _return_extras=True))
    b = SRig.pack(*r.pool.generate([r.ps[1]], r.suffixes[0][None], max_new_tokens=r.T, _return_extras=True))
    bitwise(a, b, "the same image under two keys", [r.P[1] + 9 + r.T - 1])
    held = r.m.device_bytes
    r.pool.close()
    assert r.pool.stats() == dict(slots=0, in_use=0, bytes=0, rows_gathered=0, rows_skipped=0, gather_ms=None)
    assert r.m.device_bytes < held, "the pool's memory is released"
    with pytest.raises(RuntimeError, match="pool was closed"):
        r.open("again", 0)
    with pytest.raises(RuntimeError, match="pool was closed"):
        r.pool.generate([four], r.suffixes[0][None], max_new_tokens=2)
    with pytest.raises(RuntimeError, match="gone from slot"):
        four.check()
    r.pool.close()                                     # closing twice is no error
    # a pool whose slots are too short for image 1's prefix: the store is refused, in Python and by the library
    small = r.m.session_pool(2, max_prefix_rows=r.P[0])
    with pytest.raises(ValueError, match="max_prefix_rows"):
        small.open("long", r.clip[1], r.sam[1], SIZES[1], HH[1], WW[1], r.prefix[1])
    with r.live(1):
        assert r.m.lib.anyref_session_store(r.m.h, r.m._stream(), 0) != 0 and b"max_prefix_rows" in r.m.lib.anyref_last_error(r.m.h)
    ok = small.open("short", r.clip[0], r.sam[0], SIZES[0], HH[0], WW[0], r.prefix[0])
    c = SRig.pack(*small.generate([ok], r.suffixes[0][None], max_new_tokens=r.T, _return_extras=True))
    assert c["ids"].tolist() == SRig.pack(*singles[0])["ids"].tolist()
