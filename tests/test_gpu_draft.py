"""Draft-verified greedy decode (include/anyref_hip.h `anyref_llm_extend`, `anyref_set_draft`).

1. the extend pass alone against the oracle's `llama_step` (rows appended to a KV cache), every mode, tiny and LLaMA-7B widths;
2-7. `generate` with a proposed answer in the modes whose greedy ids are pinned (parity, parity16): the output is the plain
   greedy decode whatever the draft, the counters say how it was reached;
8. the 16-bit modes, where ids are not pinned: structural invariants and the hidden rows along the oracle's ids.
"""
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from anyref_amd.config import LlmConfig, config_tiny  # noqa: E402
from anyref_amd.quant import dequantized_state_dict, dequantized_state_dict_int4  # noqa: E402
from anyref_amd.synth import synth_state_dict  # noqa: E402
from oracle import anyref_oracle as O  # noqa: E402
from test_gpu_e2e import MASK_TOL, PERF_HIDDEN_REL, PERF_HIDDEN_REL_7B, make_inputs, pad, rig_seg  # noqa: E402

F32_MODES = ("parity", "parity16", "parity16_f16")
LOGIT_TOL = {True: 2e-4, False: 1.1e-2}      # tests/test_gpu_stages.py TOL (f32-level / 16-bit), doubled for logits as there
T_NEW = 6


def build(cfg, sd, mode, **kw):
    from anyref_amd.model import AnyRefForCausalLM
    m = AnyRefForCausalLM.from_state_dict(cfg, {k: v.cuda() for k, v in sd.items()}, mode=mode, **kw)
    m.config.eos_token_id = None
    return m


def bf16_exact(sd):
    return {k: (v.bfloat16().float() if v.is_floating_point() else v) for k, v in sd.items()}


def ref_weights(sd, mode):
    return dequantized_state_dict_int4(sd) if mode == "perf_int4w" else dequantized_state_dict(sd) if mode == "perf_fp8w" else sd


# ----------------------------------------------------------------------------------------------------------------------
# 1. llm_extend against the oracle's llama_step
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extend_case(wide):
    """(cfg, sd, embeds [B, rows, H], prefixes, extensions) -- tiny: B = 2, prefixes 19 / 12, extensions 5 / 3; two layers at
    LLaMA-7B widths: B = 1, prefix 300, 9 more rows.  Weights bf16-representable: every mode sees the values the oracle sees."""
    cfg = config_tiny()
    if wide:
        cfg = dataclasses.replace(cfg, llm=LlmConfig(vocab=1000, dim=4096, heads=32, layers=2, mlp=11008, max_seq=512))
        pre, ext = [300], [9]
    else:
        pre, ext = [19, 12], [5, 3]
    sd = bf16_exact(synth_state_dict(cfg, seed=31 + wide, scale=0.02 if wide else 0.05))
    g = torch.Generator().manual_seed(32 + wide)
    rows = sd["model.embed_tokens.weight"][torch.randint(0, cfg.llm.vocab, (len(pre), max(pre) + max(ext)), generator=g)]
    return cfg, sd, rows.contiguous(), pre, ext


@functools.lru_cache(maxsize=None)
def extend_oracle(wide, which):
    """oracle hidden rows (prefix, extension) and last-row logits per sequence, on the weights `which` ("", "int4", "fp8")"""
    cfg, sd, x, pre, ext = extend_case(wide)
    w = {"": sd, "int4": dequantized_state_dict_int4(sd) if which == "int4" else None,
         "fp8": dequantized_state_dict(sd) if which == "fp8" else None}[which]
    out = []
    with torch.no_grad():
        for b in range(len(pre)):
            st = O._KVState(cfg.llm.layers)
            h0, _ = O.llama_step(w, cfg, x[b, : pre[b]], st)
            h1, _ = O.llama_step(w, cfg, x[b, pre[b]: pre[b] + ext[b]], st)
            out.append((h0, h1, F.linear(h1[-1], w["lm_head.weight"])))
    return out


def run_extend(m, wide):
    cfg, sd, x, pre, ext = extend_case(wide)
    B, n = len(pre), max(ext)
    m.llm_forward(x[:, : max(pre)], lens=pre)
    e = torch.zeros(B, n, x.shape[2])
    for b in range(B):
        e[b, : ext[b]] = x[b, pre[b]: pre[b] + ext[b]]
    return m.llm_extend(e, pre, ext, want_logits=True)


def extend_errors(r, ref, ext):
    herr = scale = lerr = lscale = 0.0
    for b, (h0, h1, lg) in enumerate(ref):
        got = r["hidden"][b].cpu()
        assert torch.isnan(got[ext[b]:]).all(), f"row {b}: rows past lens[b] must keep the sentinel"
        herr = max(herr, (got[: ext[b]] - h1).abs().max().item())
        scale = max(scale, h1.abs().max().item(), h0.abs().max().item())
        lerr = max(lerr, (r["logits"][b, ext[b] - 1].cpu() - lg).abs().max().item())
        lscale = max(lscale, lg.abs().max().item())
    return herr, scale, lerr, lscale


@pytest.mark.parametrize("wide,mode", [(0, "parity"), (0, "parity16"), (0, "perf"), (0, "perf_f16"), (0, "perf_int4w"),
                                       (0, "perf_fp8w"), (1, "perf"), (1, "parity16"), (1, "perf_int4w")])
def test_llm_extend_vs_oracle_llama_step(wide, mode):
    """llm_forward on a ragged prefix, llm_extend on the next rows: hidden rows and the last row's logits against the oracle
    appending the same rows to its cache.  Bounds: the ones the generate tests hold hidden rows to (2e-4 x max(1, scale) at f32
    level, PERF_HIDDEN_REL / _7B x scale for 16-bit operands); perf_int4w as its own test does: twice perf's error on the same
    rows with the original weights, measured here."""
    cfg, sd, x, pre, ext = extend_case(wide)
    B = len(pre)
    f32 = mode in F32_MODES
    which = {"perf_int4w": "int4", "perf_fp8w": "fp8"}.get(mode, "")
    ref = extend_oracle(wide, which)
    rel16 = PERF_HIDDEN_REL_7B if wide else PERF_HIDDEN_REL
    bound_of = lambda scale: 2e-4 * max(1.0, scale) if f32 else rel16 * scale
    if mode == "perf_int4w":
        mp = build(cfg, sd, "perf", max_batch=B)
        pe, ps, _, _ = extend_errors(run_extend(mp, wide), extend_oracle(wide, ""), ext)
        del mp
        print(f"[perf, wide={wide}] extend hidden err {pe:.3e} (scale {ps:.2f}) -> int4w bound {2 * pe:.3e}")
        bound_of = lambda scale: 2 * pe
    m = build(cfg, sd, mode, max_batch=B)
    r = run_extend(m, wide)
    herr, scale, lerr, lscale = extend_errors(r, ref, ext)
    print(f"[{mode}, wide={wide}] extend hidden err {herr:.3e} (scale {scale:.2f}, bound {bound_of(scale):.3e}); "
          f"last-row logits err {lerr:.3e} (scale {lscale:.2f})")
    assert herr <= bound_of(scale), (herr, bound_of(scale))
    assert lerr <= 2 * LOGIT_TOL[f32] * max(1.0, lscale), (lerr, lscale)
    # an extend that would pass llm_max_seq, or that names more valid rows than it brings, is refused before anything is queued
    S = cfg.llm.max_seq
    with pytest.raises(RuntimeError, match="llm_max_seq"):
        m.llm_extend(torch.zeros(B, 4, x.shape[2]), [S - 3] * B, [4] * B)
    with pytest.raises(RuntimeError, match="llm_extend"):
        m.llm_extend(torch.zeros(B, 4, x.shape[2]), [0] * B, [5] * B)      # more valid rows than rows
    r2 = run_extend(m, wide)                                                # the refusals left the handle usable
    assert torch.equal(r2["hidden"].isnan(), r["hidden"].isnan())
    assert torch.equal(torch.nan_to_num(r2["hidden"]), torch.nan_to_num(r["hidden"]))


# ----------------------------------------------------------------------------------------------------------------------
# 2 - 7. generate with a draft, ids pinned
# ----------------------------------------------------------------------------------------------------------------------
class Rig:
    """one handle + inputs + its plain answer"""

    def __init__(self, mode, B, cfg=None, sd=None, seed=3, init=None, max_seq=None, T=T_NEW, **kw):
        cfg = cfg or config_tiny()
        if max_seq:
            cfg = dataclasses.replace(cfg, llm=dataclasses.replace(cfg.llm, max_seq=max_seq))
        self.cfg, self.B, self.T = cfg, B, T
        self.sd = sd if sd is not None else (synth_state_dict(cfg, seed=seed, init=init) if init else
                                             synth_state_dict(cfg, seed=seed, scale=0.05))
        self.clip, self.sam, self.ids = make_inputs(cfg, B, seed=seed + 1)
        self.sizes, self.H, self.W = [(224, 180)] * B, [300] * B, [241] * B
        if init is None and sd is None:
            rig_seg(cfg, self.sd, self.clip, self.sam, self.ids, self.sizes, (self.H, self.W))
        self.padded, self.mask = pad(self.ids)
        self.slen = [len(r) + cfg.clip.n_patches - 1 for r in self.ids]
        self.m = build(cfg, self.sd, mode, max_batch=B, max_seg=T, **kw)

    def gen(self, draft=None, T=None):
        (ids, masks, _), ex = self.m.generate(self.clip, self.padded, self.sam, self.sizes, self.H, self.W,
                                              max_new_tokens=T or self.T, attention_masks=self.mask, _return_extras=True,
                                              draft_ids=draft)
        new = [ids[b, len(self.ids[b]): int(ex["out_lens"][b])].cpu().tolist() for b in range(self.B)]
        return dict(ids=ids.cpu(), new=new, masks=None if masks is None else [t.cpu() for t in masks], hidden=ex["hidden"].cpu(),
                    offered=ex["draft_offered"].tolist(), accepted=ex["draft_accepted"].tolist(), steps=ex["decode_steps"],
                    passes=ex["verify_passes"], low=ex["low_res"].cpu())


def same_result(a, b, what, bitwise=False, rows=None):
    assert torch.equal(a["ids"], b["ids"]), f"{what}: ids differ"
    assert (a["masks"] is None) == (b["masks"] is None), what
    for x, y in zip(a["masks"] or [], b["masks"] or []):
        assert x.shape == y.shape, what
        if bitwise:
            assert torch.equal(x, y), f"{what}: masks differ"
        elif x.numel():
            err = (x - y).abs().max().item()
            assert err <= MASK_TOL, f"{what}: mask err {err}"
    if bitwise:
        assert torch.equal(a["low"], b["low"]), f"{what}: low-res logits differ"
    for bb, n in enumerate(rows or []):
        err = (a["hidden"][bb, :n] - b["hidden"][bb, :n]).abs().max().item()
        assert err <= 2e-4, f"{what}: row {bb} hidden err {err}"


@functools.lru_cache(maxsize=None)
def rig(mode, B):
    r = Rig(mode, B)
    r.plain = r.gen()
    assert r.plain["steps"] == T_NEW - 1 and r.plain["passes"] == 0 and r.plain["offered"] == [0] * B
    assert r.plain["masks"] is not None and all(len(t) == T_NEW for t in r.plain["new"])
    print(f"[{mode} B={B}] plain answer: {r.plain['new']}")
    return r


@pytest.mark.parametrize("mode", ["parity", "parity16"])
@pytest.mark.parametrize("B", [1, 2])
def test_true_draft_is_accepted_in_one_pass(mode, B):
    r = rig(mode, B)
    d = r.gen(draft=[t[:5] for t in r.plain["new"]])
    assert d["offered"] == [5] * B and d["accepted"] == [5] * B, d
    assert d["steps"] == 0 and d["passes"] == 1
    same_result(d, r.plain, "true draft", rows=[s + 5 for s in r.slen])
    # the [B, K] tensor form, rows closed by a negative id
    t = torch.full((B, 9), -1, dtype=torch.long)
    for b in range(B):
        t[b, :5] = torch.tensor(r.plain["new"][b][:5])
    d2 = r.gen(draft=t)
    assert d2["accepted"] == [5] * B
    same_result(d2, d, "tensor form", bitwise=True)


@pytest.mark.parametrize("mode", ["parity", "parity16"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("at", [0, 2])
def test_wrong_draft_falls_back(mode, B, at):
    """row 0's draft corrupted at index `at`; at B = 2 row 1 keeps the true draft: ragged acceptance"""
    r = rig(mode, B)
    drafts = [list(t[:5]) for t in r.plain["new"]]
    drafts[0][at] = (drafts[0][at] + 1) % r.cfg.llm.vocab
    d = r.gen(draft=drafts)
    want = [at] + [5] * (B - 1)
    assert d["accepted"] == want, d
    assert d["steps"] == 5 - min(want)
    assert d["passes"] == (0 if (B == 1 and at == 0) else 1)
    assert d["offered"] == ([0 if at == 0 else 5] + [5] * (B - 1))
    same_result(d, r.plain, f"draft wrong at {at}", rows=[s + 5 for s in r.slen])


def test_eos_inside_the_draft_and_cut_drafts():
    r = rig("parity", 1)
    new = r.plain["new"][0]
    V = r.cfg.llm.vocab
    # drafts that are cut: an id < 0, an id >= vocab, 40 tokens
    for draft, offered in (([new[0], new[1], -1, new[3], new[4]], 2), ([new[0], V, new[2]], 1),
                           (new[:5] + [(new[5] + 1 + i) % V for i in range(35)], 5)):
        d = r.gen(draft=[draft])
        assert d["offered"] == [offered] and d["accepted"] == [offered], (draft, d["offered"], d["accepted"])
        assert d["steps"] == 5 - offered
        same_result(d, r.plain, f"cut draft {draft[:6]}", rows=[r.slen[0] + 5])
    # EOS = the id emitted at step 3: a draft that runs past it ends where the plain run with that EOS ends
    r.m.config.eos_token_id = new[3]
    try:
        p = r.gen()
        stop = new.index(new[3])
        assert p["new"][0] == new[: stop + 1]
        d = r.gen(draft=[new[:5]])
        assert d["accepted"] == [5] and d["steps"] == 0
        same_result(d, p, "EOS inside the draft", rows=[r.slen[0] + stop])
    finally:
        r.m.config.eos_token_id = None


def test_cache_limit_in_a_batch():
    """B = 2, row 0 at slen + max_new_tokens == max_seq: nothing of its draft may be fed (a row that gets ahead keeps stepping
    while the other finishes); row 1, three rows shorter, is fed 3 tokens"""
    cfg = config_tiny()
    slen0 = 16 + cfg.clip.n_patches - 1
    r = Rig("parity", 2, max_seq=slen0 + T_NEW)
    assert r.slen == [slen0, slen0 - 3]
    p = r.gen()
    d = r.gen(draft=[t[:5] for t in p["new"]])
    assert d["offered"] == [0, 3] and d["accepted"] == [0, 3] and d["passes"] == 1 and d["steps"] == 5, d
    same_result(d, p, "cache limit", rows=[s + 5 for s in r.slen])


def test_scheduling_and_fallback():
    r = Rig("parity", 1, seed=5, init="fan_in")          # O(1) logits: a varied greedy answer
    m = r.m
    m.set_early_tail(False)
    p0 = r.gen()
    new = p0["new"][0]
    prompt = set(r.padded[0].tolist())
    once = [t for t in new[:5] if new.count(t) == 1 and t not in prompt]
    assert once, new
    m.set_seg_token_idx(int(once[0]))                    # exactly one [SEG]: one prompt per mask-decoder call on both tail paths
    plain = r.gen()
    assert plain["masks"] is not None and plain["masks"][0].shape[0] == 1
    runs = {}
    for early in (False, True):
        for graphs in (False, True):
            m.set_early_tail(early); m.set_graphs(graphs)
            runs[early, graphs] = d = r.gen(draft=[new[:3]])     # 3 accepted, 2 steps behind the pass
            assert d["accepted"] == [3] and d["steps"] == 2 and d["passes"] == 1
    for k, d in runs.items():
        same_result(d, runs[False, False], f"early, graphs = {k}", bitwise=True)
        assert torch.equal(d["hidden"], runs[False, False]["hidden"])
    same_result(runs[True, True], plain, "draft vs plain", rows=[r.slen[0] + 5])
    m.set_early_tail(False)
    # no stale one-shot: a plain call after a draft call is the plain call before it, bit for bit
    after = r.gen()
    assert after["offered"] == [0] and after["passes"] == 0 and after["steps"] == 5
    same_result(after, plain, "plain after draft", bitwise=True)
    assert torch.equal(after["hidden"], plain["hidden"])
    # set_draft, then a teacher-forced forward: nothing stays armed
    m.set_draft([new[:5]])
    full = plain["ids"][0]
    labels = full.clone()
    labels[: len(r.ids[0])] = -100
    m.model_forward_new(r.clip, r.sam, full[None], labels[None], None, r.sizes, None, r.H, r.W)
    after = r.gen()
    assert after["offered"] == [0] and after["passes"] == 0 and after["steps"] == 5
    same_result(after, plain, "plain after set_draft + forward", bitwise=True)
    # a draft for another batch size is refused, and the refusal consumes it
    m2 = Rig("parity", 2, seed=5, init="fan_in")
    m2.m.set_draft([new[:5]])
    with pytest.raises(RuntimeError, match="batch size"):
        m2.gen()
    assert m2.gen()["offered"] == [0, 0]


def test_rephrase_ignores_the_draft():
    cfg = config_tiny()
    cfg.rephrase_weight = 0.5
    r = Rig("parity", 1, cfg=cfg, seed=7)
    p = r.gen()
    d = r.gen(draft=[p["new"][0][:5]])
    assert d["offered"] == [0] and d["passes"] == 0 and d["steps"] == 5
    same_result(d, p, "rephrase", bitwise=True)


def test_policy_last():
    r = rig("parity", 1)
    m = r.m
    m.set_draft_policy("last")
    try:
        a = r.gen()
        b = r.gen()
        assert a["offered"] == [0] and b["accepted"] == [T_NEW - 1] and b["steps"] == 0
        same_result(b, a, "policy last", rows=[r.slen[0] + 5])
        m.set_draft_policy(None)
        c = r.gen()
        assert c["offered"] == [0] and c["passes"] == 0
        same_result(c, a, "policy off", bitwise=True)
    finally:
        m.set_draft_policy(None)


# ----------------------------------------------------------------------------------------------------------------------
# 8. 16-bit modes: ids are not pinned
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_case(wide, int4):
    cfg = config_tiny()
    if wide:
        cfg = dataclasses.replace(cfg, llm=LlmConfig(vocab=1000, dim=4096, heads=32, layers=2, mlp=11008, max_seq=512))
    sd = bf16_exact(synth_state_dict(cfg, seed=21, scale=0.02 if wide else 0.05))
    w = dequantized_state_dict_int4(sd) if int4 else sd
    clip, sam, ids = make_inputs(cfg, 1, seed=22, L=65 if wide else 16)
    sizes, H, W = [(224, 224)], [224], [224]
    rig_seg(cfg, w, clip, sam, ids, sizes, (H, W))
    with torch.no_grad():
        ref = O.anyref_generate(w, cfg, clip, ids, sam, sizes, H, W, max_new_tokens=T_NEW, eos=False)
    return cfg, sd, (clip, sam, ids, sizes, H, W), ref


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("mode", ["perf", "perf_int4w"])
def test_draft_in_16_bit_modes(mode, wide):
    """The oracle's answer as the draft.  The pass and the step run different kernels on 16-bit operands and the project pins no
    greedy ids in these modes, so the acceptance count is printed, not asserted; what holds whatever was accepted: the output
    follows the draft on [0, accepted) and leaves it at `accepted`, the step count, and the hidden rows computed along the
    oracle's ids against the oracle's (the generate tests' 16-bit bound)."""
    cfg, sd, (clip, sam, ids, sizes, H, W), ref = oracle_case(wide, mode == "perf_int4w")
    m = build(cfg, sd, mode, max_batch=1, max_seg=T_NEW)
    L = len(ids[0])
    want = ref["output_ids"][0][L:].tolist()
    draft = want[:5]
    (out, _, _), ex = m.generate(clip, ids[0][None], sam, sizes, H, W, max_new_tokens=T_NEW, _return_extras=True, draft_ids=[draft])
    got = out[0, L:].cpu().tolist()
    off, acc = int(ex["draft_offered"][0]), int(ex["draft_accepted"][0])
    print(f"[{mode}, wide={wide}] offered {off}, accepted {acc}, decode steps {ex['decode_steps']}; ids {got} (oracle {want})")
    assert len(got) == T_NEW and 0 <= acc <= off <= 5
    assert got[:acc] == draft[:acc]
    if off and acc < off:
        assert got[acc] != draft[acc]
    assert ex["decode_steps"] == T_NEW - 1 - acc
    assert ex["verify_passes"] == (1 if off else 0)
    slen = L + cfg.clip.n_patches - 1
    n = slen + acc
    hw = ref["hidden"][0][:n]
    scale = hw.abs().max().item()
    err = (ex["hidden"][0, :n].cpu() - hw).abs().max().item()
    rel = PERF_HIDDEN_REL_7B if wide else PERF_HIDDEN_REL
    print(f"[{mode}, wide={wide}] hidden rows [0, {n}) err {err:.3e} (scale {scale:.2f}, bound {rel * max(1.0, scale):.3e})")
    assert err < rel * max(1.0, scale)
