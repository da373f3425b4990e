"""SAM spatial prompts through the model (include/anyref_hip.h `anyref_prompt_reserve` / `anyref_mask_decode_prompted` /
`anyref_refine_masks`): the prompted decoder against the CPU rule + oracle and the reference's own outputs
(tests/golden/sam_prompts.npz), the text-only path bit for bit, refine after generate / a session / a pooled call, refusals, and
what a handle that reserves nothing holds.  The decoder is f32 in both modes; its tolerance is the project's decoder figure."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prompts as gp  # noqa: E402
from anyref_amd import prompts as P  # noqa: E402
from anyref_amd.config import config_tiny  # noqa: E402
from anyref_amd.synth import synth_state_dict, synth_prompt_weights  # noqa: E402
from oracle import anyref_oracle as O  # noqa: E402
from test_gpu_draft import Rig, T_NEW  # noqa: E402
from test_gpu_e2e import make_inputs, rig_seg  # noqa: E402
from test_gpu_stages import build, close  # noqa: E402

MODES = ["parity", "perf"]
DEC_TOL = 2e-4          # tests/test_gpu_stages.py: x max(1, max |ref|)
FX = np.load(os.path.join(HERE, "golden", "sam_prompts.npz"))
SEED = int(FX["seed"])
POST = gp.POST_SIZES


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def stage(mode):
    """one sam_w14 handle with the spatial weights, reserved for 4 points; the fixture's inputs"""
    cfg, sd = gp.cfg(), gp.prompt_weights(SEED)
    emb, sets = gp.prompt_inputs(SEED)
    m = build(cfg, sd, mode, max_batch=1, max_seg=3)
    m.set_spatial_prompts(4)
    return cfg, sd, emb, sets, m


# ---- 1. every fixture prompt set against the rule + oracle and against the reference ---------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", gp.SETS)
def test_mask_decode_prompted(mode, name):
    cfg, sd, emb, sets, m = stage(mode)
    a = sets[name]
    sparse, dense = P.encode(sd, cfg, **a)
    with torch.no_grad():
        m4_ref, iou_ref = O.mask_decoder_predict(sd, cfg, emb, O.dense_pe(sd, cfg), sparse.float(), dense.float())
        tok, best_ref = P.pick(iou_ref, True)
        post_ref = O.postprocess_masks(cfg, m4_ref[:, tok], *POST)
    r = m.mask_decode(emb[0], a["text"], POST[0], POST[1], points=a["points"], point_labels=a["labels"], boxes=a["boxes"],
                      mask_input=a["mask_input"], multimask_output=True)
    close(r["masks4"], m4_ref, DEC_TOL, f"{name}: masks vs rule + oracle")
    close(r["iou"], iou_ref, DEC_TOL, f"{name}: iou vs rule + oracle")
    close(r["iou"], FX[f"{name}_iou"], DEC_TOL, f"{name}: iou vs reference golden")
    close(r["masks"], post_ref, DEC_TOL, f"{name}: multimask postprocess vs oracle")
    assert r["masks"].shape == (3, 3, *POST[1]) and torch.equal(bits(r["low_res"]), bits(r["masks4"][:, 1:4]))
    assert r["best"].tolist() == best_ref.tolist() == FX[f"{name}_best"].tolist()
    if name == "all":
        close(r["masks4"][:, :, ::2, ::2], FX["all_masks4"], DEC_TOL, "all: predict_masks vs reference golden")
        close(r["masks"][:, :, ::8, ::8], FX["all_post"], DEC_TOL, "all: postprocess vs reference golden")
    one = m.mask_decode(emb[0], a["text"], POST[0], POST[1], points=a["points"], point_labels=a["labels"], boxes=a["boxes"],
                        mask_input=a["mask_input"])
    assert torch.equal(bits(one["masks4"]), bits(r["masks4"])) and one["masks"].shape == (3, *POST[1])
    close(one["masks"], O.postprocess_masks(cfg, m4_ref[:, 0:1], *POST)[:, 0], DEC_TOL, f"{name}: token 0 postprocess")


# ---- 2. text only through the prompted entry -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_text_only_is_bit_identical(mode):
    cfg, sd, emb, sets, m = stage(mode)
    text = sets["text"]["text"]
    plain = m.mask_decode(emb[0], text, POST[0], POST[1])
    # multimask_output=False and no prompt at all would take the plain entry: go through the prompted one by hand
    r = m._mask_decode_prompted(emb[0], text, POST[0], POST[1], None, None, None, None, False)
    for k in ("masks4", "iou", "masks"):
        assert torch.equal(bits(r[k]), bits(plain[k])), f"text only through anyref_mask_decode_prompted: {k} differs"
    again = m.mask_decode(emb[0], text, POST[0], POST[1])
    assert torch.equal(bits(again["masks4"]), bits(plain["masks4"])), "the prompted pass changed the plain path"


# ---- 3. refine after generate ----------------------------------------------------------------------------------------
def seg_rig(mode, spatial=True):
    """the tiny config rigged to answer with [SEG] (tests/test_gpu_draft.py), its state dict with the spatial weights"""
    cfg = config_tiny()
    sd = synth_state_dict(cfg, seed=3, scale=0.05)
    clip, sam, ids = make_inputs(cfg, 1, seed=4)
    rig_seg(cfg, sd, clip, sam, ids, [(224, 180)], ([300], [241]))
    if spatial:
        sd.update(synth_prompt_weights(cfg, seed=3))
    return Rig(mode, 1, cfg=cfg, sd=sd)


def one_seg_T(r):
    """new tokens up to and including the first [SEG]: a call whose row has exactly one mask, decoded alone"""
    d = r.gen()
    lo, hi = r.cfg.seg_range()
    seg = [i for i, t in enumerate(d["new"][0]) if lo <= t <= hi]
    assert seg, f"the rig's answer {d['new']} has no [SEG]"
    return seg[0] + 1


BOX = torch.tensor([40.0, 60.0, 200.0, 250.0])              # original pixels of the rigs' 300 x 241 images
SIZE, HW_ = (224, 180), (300, 241)


def stage_check(m, cfg, sd, z, emb, pred, low, what):
    """z = refine(row, seg, box=BOX, mask_input=True, multimask_output=True) against the stage entry: `mask_decode` of the
    same prompts on `sam_encode`'s embedding `emb` [1,C,g,g] and the call's own [SEG] embedding `pred` (refine_embedding),
    BIT FOR BIT; and against the rule + oracle at the decoder tolerance"""
    box_in = P.to_input_frame(BOX.reshape(2, 2), HW_, SIZE).reshape(1, 4)
    low = low.reshape(1, *low.shape[-2:])
    q = m.mask_decode(emb[0], pred[None], SIZE, HW_, boxes=box_in, mask_input=low, multimask_output=True)
    assert torch.equal(bits(q["low_res"][0]), bits(z["low_res"])), f"{what}: low-res logits differ from mask_decode's"
    assert torch.equal(bits(q["masks"][0]), bits(z["masks"])), f"{what}: masks differ from mask_decode's"
    assert torch.equal(bits(q["iou"][0, 1:4]), bits(z["iou"])) and int(q["best"][0]) == z["best"], f"{what}: iou / best"
    with torch.no_grad():
        sparse, dense = P.encode(sd, cfg, None, None, box_in, low.cpu(), pred.cpu()[None])
        m4_ref, iou_ref = O.mask_decoder_predict(sd, cfg, emb.cpu(), O.dense_pe(sd, cfg), sparse.float(), dense.float())
        post_ref = O.postprocess_masks(cfg, m4_ref[:, 1:4], SIZE, HW_)[0]
    close(z["low_res"], m4_ref[0, 1:4], DEC_TOL, f"{what}: refine(box, mask) vs rule + oracle")
    close(z["masks"], post_ref, DEC_TOL, f"{what}: refine masks vs oracle")
    close(z["iou"], iou_ref[0, 1:4], DEC_TOL, f"{what}: refine iou vs oracle")
    assert z["best"] == int(P.pick(iou_ref, True)[1][0]) or \
        float(iou_ref[0, 1:4].topk(2).values.diff().abs()) < 50 * DEC_TOL, f"{what}: best"


@pytest.mark.parametrize("mode", MODES)
def test_refine_after_generate(mode):
    """refine without a prompt is the call's mask and low-res logits bit for bit (early masks on and off); refine(box,
    mask_input=True) is `mask_decode` of the same prompts on `sam_encode`'s embedding and the call's [SEG] embedding bit for
    bit, and the rule + oracle within the decoder tolerance; a plain generate without extras feeds refine the same logits; a
    later generate is a fresh handle's bit for bit."""
    fresh = seg_rig(mode)
    T = one_seg_T(fresh)
    first = fresh.gen(T=T)                       # (what a handle that never refined answers)
    r = seg_rig(mode)
    m = r.m
    m.set_spatial_prompts(4)
    cfg, sd = r.cfg, r.sd
    for early in (True, False):
        m.set_early_tail(early)
        d = r.gen(T=T)
        assert len(d["masks"][0]) == 1
        z = m.refine(0, 0)
        assert torch.equal(bits(z["masks"][0].cpu()), bits(d["masks"][0][0])), f"early={early}: refine without a prompt, mask"
        assert torch.equal(bits(z["low_res"][0].cpu()), bits(d["low"][0, 0])), f"early={early}: ... low-res logits"
        z = m.refine(0, 0, box=BOX, mask_input=True, multimask_output=True)
        pred = m.refine_embedding(0, 0)
        # the same refine after a plain call WITHOUT extras: the low-res logits are kept because prompts are reserved
        ids2, masks2, _ = m.generate(r.clip, r.padded, r.sam, r.sizes, r.H, r.W, max_new_tokens=T, attention_masks=r.mask)
        assert torch.equal(bits(masks2[0].cpu()), bits(d["masks"][0]))
        z2 = m.refine(0, 0, box=BOX, mask_input=True, multimask_output=True)
        for k in ("masks", "low_res", "iou"):
            assert torch.equal(bits(z2[k]), bits(z[k])), f"early={early}: refine after a call without extras, {k}"
        emb = m.sam_encode(r.sam)                                   # (ends the refine: asserted below)
        with pytest.raises(RuntimeError, match="refine lost: ended by anyref_sam_encode"):
            m.refine(0, 0)
        with pytest.raises(RuntimeError, match="refine lost: ended by anyref_sam_encode"):
            m.refine_embedding(0, 0)
        stage_check(m, cfg, sd, z, emb, pred, d["low"][0, 0].cuda(), f"early={early}")
    m.set_early_tail(True)
    nxt = r.gen(T=T)
    assert torch.equal(nxt["ids"], first["ids"]) and torch.equal(bits(nxt["low"]), bits(first["low"]))
    assert torch.equal(bits(nxt["masks"][0]), bits(first["masks"][0])), "a generate after refines differs from a fresh handle's"


# ---- 5 / 6. refusals and bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity"])
def test_refusals_and_bytes(mode):
    plain, with_w = seg_rig(mode, spatial=False), seg_rig(mode)
    sp_bytes = sum(v.numel() * 4 for k, v in with_w.sd.items() if k[len(P.PE_PREFIX):] in P.SPATIAL_NAMES)
    gauss = with_w.cfg.sam.out_chans * 4          # the Gaussian matrix is kept beside them (dense_pe holds its sines only)
    assert with_w.m.device_bytes - plain.m.device_bytes == sp_bytes + gauss, "unreserved: the weights' own bytes and no more"
    with pytest.raises(RuntimeError, match="missing weight: .*point_embeddings.0.weight"):
        plain.m.set_spatial_prompts(4)
    m = with_w.m
    T = one_seg_T(with_w)
    d = with_w.gen(T=T)
    sp = m._spatial(1, None, None, None, None, False)[0]
    out = torch.full((300 * 241,), 7.0, device="cuda")

    def refused(rc, text):
        torch.cuda.synchronize()
        assert rc != 0 and text in m.lib.anyref_last_error(m.h).decode(), m.lib.anyref_last_error(m.h).decode()
        assert bool((out == 7.0).all()), "a refused call wrote its output"
    call = lambda row, seg, s: m.lib.anyref_refine_masks(m.h, None, row, seg, C.byref(s), None, None, C.c_void_p(out.data_ptr()))
    refused(call(0, 0, sp), "not reserved")
    base = m.device_bytes
    m.set_spatial_prompts(2)
    grown = m.device_bytes
    assert grown > base
    m.set_spatial_prompts(2)
    assert m.device_bytes == grown, "the same reservation again changes nothing"
    refused(call(0, 0, sp), "refine lost: ended by anyref_prompt_reserve")
    d2 = with_w.gen(T=T)
    assert torch.equal(bits(d2["low"]), bits(d["low"]))
    refused(call(0, 1, sp), "seg outside")
    refused(call(1, 0, sp), "row outside")
    pts = torch.zeros(1, 3, 2)
    sp3 = m._spatial(1, pts, torch.ones(1, 3, dtype=torch.int32), None, None, False)
    refused(call(0, 0, sp3[0]), "n_points 3 outside")
    sp3[0].n_points, sp3[0].labels = 1, None
    refused(call(0, 0, sp3[0]), "without labels")
    z = m.refine(0, 0)                                      # the state is intact: the refine still answers
    assert torch.equal(bits(z["low_res"][0].cpu()), bits(d2["low"][0, 0]))
    m.set_spatial_prompts(0)
    assert m.device_bytes == base, "reserve(0) frees the workspaces"


# ---- 4. the same through an image session and one pooled call of two slots -------------------------------------------
@pytest.mark.parametrize("mode", ["parity"])
def test_refine_in_a_session_and_a_pool(mode):
    from anyref_amd.config import IMAGE_TOKEN_INDEX
    from test_gpu_draft import build as dbuild
    cfg = config_tiny()
    sd = synth_state_dict(cfg, seed=3, scale=0.05)
    clip, sam, ids = make_inputs(cfg, 1, seed=4)
    H, W = HW_
    rig_seg(cfg, sd, clip, sam, ids, [SIZE], ([H], [W]))
    sd.update(synth_prompt_weights(cfg, seed=3))
    m = dbuild(cfg, sd, mode, max_batch=2, max_seg=T_NEW)
    m.set_spatial_prompts(4)
    row = ids[0]
    prefix = row[: row.tolist().index(IMAGE_TOKEN_INDEX) + 1]
    (out, _, _), ex = m.generate(clip, row[None], sam, [SIZE], [H], [W], max_new_tokens=T_NEW, _return_extras=True)
    lo, hi = cfg.seg_range()
    new = out[0, len(row): int(ex["out_lens"][0])].tolist()
    T = [i for i, t in enumerate(new) if lo <= t <= hi][0] + 1          # exactly one [SEG] per row
    # a second SAM image: the answer (CLIP + LLaMA) is the same, the mask is not
    sam_b = torch.randn(sam.shape, generator=torch.Generator().manual_seed(99))
    embs = [m.sam_encode(sam), m.sam_encode(sam_b)]

    def same(z, masks, low, what):
        assert torch.equal(bits(z["masks"][0]), bits(masks)) and torch.equal(bits(z["low_res"][0]), bits(low)), what

    with m.image_session(clip[0], sam[0], SIZE, H, W, prefix) as s:
        for extras in (True, False):             # False: the logits are kept only because prompts are reserved
            r = s.generate(row[None], max_new_tokens=T, _return_extras=extras)
            (o, masks, _), low = (r[0], r[1]["low_res"][0, 0]) if extras else (r, low)
            assert masks[0].shape[0] == 1
            same(s.refine(0, 0), masks[0][0], low, f"session (extras {extras}): refine without a prompt")
            z = s.refine(0, 0, box=BOX, mask_input=True, multimask_output=True)
            stage_check(m, cfg, sd, z, embs[0], m.refine_embedding(0, 0), low, f"session (extras {extras})")
        (o2, masks2, _), _ = s.generate(row[None], max_new_tokens=T, _return_extras=True)        # the session still answers
        assert torch.equal(o, o2) and torch.equal(bits(masks[0]), bits(masks2[0])), "a session query after refines differs"
    pool = m.session_pool(2)
    a = pool.open("a", clip[0], sam[0], SIZE, H, W, prefix)
    b = pool.open("b", clip[0], sam_b[0], SIZE, H, W, prefix)
    rows = torch.stack([row, row])
    (o, masks, _), ex = pool.generate([a, b], rows, max_new_tokens=T, _return_extras=True)
    assert not torch.equal(masks[0], masks[1]), "the two slots hold different images"
    zs = []
    for q in (0, 1):
        same(m.refine(q, 0), masks[q][0], ex["low_res"][q, 0], f"pooled call: row {q}")
        zs.append(m.refine(q, 0, box=BOX, mask_input=True, multimask_output=True))
        stage_check(m, cfg, sd, zs[q], embs[q], m.refine_embedding(q, 0), ex["low_res"][q, 0], f"pooled call: row {q}")
    assert not torch.equal(zs[0]["masks"], zs[1]["masks"]), "row 1 was refined on row 0's image"
    (o2, masks2, _), _ = pool.generate([a, b], rows, max_new_tokens=T, _return_extras=True)      # the slots still answer
    assert torch.equal(o, o2) and all(torch.equal(bits(x), bits(y)) for x, y in zip(masks, masks2))
    pool.close()


# ---- a model built the deferred way (from_pretrained's flow) ---------------------------------------------------------
def test_set_spatial_prompts_first_on_a_deferred_model():
    """`from_pretrained` gathers weights on the host and builds the handle at the first call that needs it: that call may
    be set_spatial_prompts"""
    from anyref_amd.model import AnyRefForCausalLM
    cfg = config_tiny()
    sd = synth_state_dict(cfg, seed=3, scale=0.05)
    sd.update(synth_prompt_weights(cfg, seed=3))
    m = AnyRefForCausalLM(cfg, mode="parity", defer=True, max_seg=2)
    m.load_state_dict(sd)
    assert m.h is None
    m.set_spatial_prompts(4)                     # before anything else
    assert m.h is not None and m._sp_max == 4
    with pytest.raises(RuntimeError, match="no generating call"):
        m.refine_embedding(0, 0)
    m2 = AnyRefForCausalLM(cfg, mode="parity", defer=True, max_seg=2)
    m2.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="spatial prompts are not reserved"):
        m2.refine(0, 0)                          # builds the handle, then refuses: nothing is reserved
    assert m2.h is not None
