"""ANYREF_MODE_PARITY16_F16 (Python mode="parity16_f16") end to end: the tolerance-meeting arithmetic on an fp16 checkpoint held
bit for bit.

Weights are made as tests/test_gpu_perf_f16.py makes them: seeded, rounded once to f16, handed over as fp16 tensors -- what a
user's fp16 checkpoint (the reference's evaluation dtype) is.  The oracle is the CPU fp32 forward on those f16 values widened
to f32.  north_star's bar applies: identical greedy ids, mask logits within 1e-3.  `parity16` on the same weights rounds them
to bf16 (anyref_inexact_weights > 0) and runs beside the new mode where the comparison is the point."""
import dataclasses
import gc
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from anyref_amd.config import config_tiny, config_7b, LlmConfig  # noqa: E402
from oracle import anyref_oracle as O  # noqa: E402
from oracle.check import compare_generate, summarize  # noqa: E402
from test_gpu_e2e import make_inputs, pad, rig_seg  # noqa: E402
from test_gpu_perf_f16 import build, f16_weights, f32  # noqa: E402

MODE = "parity16_f16"
MASK_TOL = 1e-3     # north_star
GIB = 1 << 30


@pytest.mark.parametrize("window,sam_dim,sam_heads", [(14, 192, 3), (4, 128, 2), (14, 320, 4)])  # last: hd 80, 196-token windows
def test_generate_matches_oracle(window, sam_dim, sam_heads):
    """config_tiny (its 688-wide MLP is not a multiple of the 64-column pair blocks: padded rows) against the oracle"""
    cfg = config_tiny(window=window, sam_dim=sam_dim, sam_heads=sam_heads)
    sd = f16_weights(cfg, seed=3, scale=0.05)
    sd32 = f32(sd)
    clip, sam, ids = make_inputs(cfg, 1, seed=4)
    sizes, H, W = [(224, 180)], [300], [241]
    rig_seg(cfg, sd32, clip, sam, ids, sizes, (H, W))
    with torch.no_grad():
        ref = O.anyref_generate(sd32, cfg, clip, ids, sam, sizes, H, W, max_new_tokens=6, eos=False)
    assert ref["pred_masks"] is not None
    m = build(cfg, sd, MODE, max_batch=1, max_seg=4)
    assert m.inexact_weights == 0
    assert "f16 pairs" in m.lib.anyref_mode_name(m.h).decode()
    (out_ids, masks, rest), ex = m.generate(clip, ids[0][None], sam, sizes, H, W, max_new_tokens=6, _return_extras=True)
    assert out_ids[0].cpu().tolist() == ref["output_ids"][0].tolist(), "greedy ids differ"
    n = ref["hidden"][0].shape[0]
    herr = (ex["hidden"][0, :n].cpu() - ref["hidden"][0]).abs().max().item()
    print(f"[{MODE}] hidden max-abs-err {herr:.3e} (scale {ref['hidden'][0].abs().max().item():.2f})")
    assert herr < 2e-4
    r = compare_generate(m, ref, clip, ids[0], sam, sizes, H, W, 6, sd32["lm_head.weight"], cfg.clip.n_patches)
    print(f"[{MODE}] " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()))
    assert r["greedy_ids_identical"] and r["mask_logit_max_abs_err"] <= MASK_TOL, r


def test_tiny_generate_audio_and_rephrase():
    """config_tiny with an audio reference whose raw mel goes through the HIP ImageBind trunk, and the rephrase branch, against
    the oracle fed the trunk's own embedding: identical greedy ids, mask logits within 1e-3"""
    from anyref_amd.config import AudioTrunkConfig, IMAGE_TOKEN_INDEX, AUDIO_REF_INDEX
    cfg = config_tiny()
    cfg.audio_trunk = AudioTrunkConfig(dim=64, blocks=2, heads=4)
    cfg.rephrase_weight = 0.5
    sd = f16_weights(cfg, seed=41, scale=0.05)
    sd32 = f32(sd)
    g = torch.Generator().manual_seed(42)
    clip = torch.randn(1, 3, 224, 224, generator=g)
    sam = torch.randn(1, 3, 224, 224, generator=g)
    body = torch.randint(3, 980, (12,), generator=g)
    ids = torch.cat([torch.tensor([1, IMAGE_TOKEN_INDEX]), body[:3], torch.full((3,), AUDIO_REF_INDEX), body[3:]])
    mel = torch.randn(1, 3, 1, 128, 204, generator=g)
    sizes, H, W = [(224, 200)], [180], [160]
    m = build(cfg, sd, MODE, max_batch=1, max_seg=8)
    assert m.inexact_weights == 0
    emb = m.audio_encode(mel).cpu()
    with torch.no_grad():
        r0 = O.anyref_generate(sd32, cfg, clip, [ids], sam, sizes, H, W, audio_embeds=[emb], max_new_tokens=4, eos=False)
        cfg.seg_token_idx = int(r0["output_ids"][0][-2])
        ref = O.anyref_generate(sd32, cfg, clip, [ids], sam, sizes, H, W, audio_embeds=[emb], max_new_tokens=5, eos=False)
    m.set_seg_token_idx(cfg.seg_token_idx)
    r = compare_generate(m, ref, clip, ids, sam, sizes, H, W, 5, sd32["lm_head.weight"], cfg.clip.n_patches, audios=[mel])
    print(f"{MODE} tiny generate (audio through the HIP trunk, rephrase 0.5): " + json.dumps(r))
    assert r["greedy_ids_identical"], r
    assert r["mask_logit_max_abs_err"] <= MASK_TOL, r


def test_ragged_batch_and_teacher_forward():
    cfg = config_tiny()
    sd = f16_weights(cfg, seed=7, scale=0.05)
    sd32 = f32(sd)
    clip, sam, ids = make_inputs(cfg, 2, seed=8)
    sizes, H, W = [(224, 224), (200, 224)], [224, 260], [224, 300]
    rig_seg(cfg, sd32, clip, sam, ids, sizes, (H, W))
    with torch.no_grad():
        ref = O.anyref_generate(sd32, cfg, clip, ids, sam, sizes, H, W, max_new_tokens=5, eos=False)
    m = build(cfg, sd, MODE, max_batch=2, max_seg=4)
    padded, mask = pad(ids)
    out_ids, masks, _ = m.generate(clip, padded, sam, sizes, H, W, max_new_tokens=5, attention_masks=mask)
    for b in range(2):
        want = ref["output_ids"][b]
        assert out_ids[b, : len(want)].cpu().tolist() == want.tolist(), f"row {b}: greedy ids differ"
        if ref["pred_masks"][b] is not None and ref["pred_masks"][b].numel():
            err = (masks[b].cpu() - ref["pred_masks"][b]).abs().max().item()
            print(f"[{MODE}] batch row {b}: mask max-abs-err {err:.3e}")
            assert err <= MASK_TOL
    # teacher-forced twin on the oracle's own ids
    full = ref["output_ids"][0]
    labels = full.clone()
    labels[: len(ids[0])] = -100
    nseg = ref["pred_masks"][0].shape[0]
    gt = [(torch.rand(nseg, H[0], W[0]) > 0.5).float()]
    with torch.no_grad():
        fr = O.anyref_forward(sd32, cfg, clip[:1], sam[:1], [full], [labels], sizes[:1], gt, H[:1], W[:1])
    out = m.model_forward_new(clip[:1], sam[:1], full[None], labels[None], None, sizes[:1], gt, H[:1], W[:1], _return_extras=True)
    assert abs(float(out["lm_loss"]) - float(fr["lm_loss"])) < 1e-3
    perr = (out["pred_masks"][0].cpu() - fr["pred_masks"][0]).abs().max().item()
    print(f"[{MODE}] teacher-forced mask max-abs-err {perr:.3e}")
    assert perr <= MASK_TOL, f"forward mask err {perr}"


@pytest.mark.parametrize("B", [1, 2])
def test_decode_launch_modes_bit_identical(B):
    cfg = config_tiny()
    sd = f16_weights(cfg, seed=5, scale=0.05)
    clip, sam, ids = make_inputs(cfg, B, seed=6, L=16)
    ids_p, _ = pad(ids)
    sizes, H, W = [(224, 224)] * B, [224] * B, [224] * B
    m = build(cfg, sd, MODE, max_batch=B, max_seg=4)
    m.set_graphs(False)
    m.set_early_tail(False)
    out0, _, _ = m.generate(clip, ids_p, sam, sizes, H, W, max_new_tokens=5)
    m.set_seg_token_idx(int(out0[0, ids_p.shape[1] + 2]))
    ref = None
    for overlap in (False, True):
        for graphs in (False, True):
            m.set_overlap(overlap); m.set_graphs(graphs)
            (o_ids, masks, _), ex = m.generate(clip, ids_p, sam, sizes, H, W, max_new_tokens=12, _return_extras=True)
            cur = (o_ids.cpu(), ex["hidden"].cpu(), [None if t is None else t.cpu() for t in masks])
            if ref is None:
                ref = cur
                assert ref[2][0] is not None
                continue
            tag = f"overlap={overlap} graphs={graphs}"
            assert torch.equal(cur[0], ref[0]), f"ids differ ({tag})"
            assert torch.equal(cur[1], ref[1]), f"hidden states differ ({tag})"
            for a, b in zip(cur[2], ref[2]):
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), f"masks differ ({tag})"


@pytest.mark.parametrize("B", [1, 4, 6])
def test_llama7b_shaped_layers_vs_oracle_and_parity16(B):
    """Two decoder layers at LLaMA-7B's widths behind the tiny towers, f16 weights, every hidden state against the CPU fp32
    oracle in parity16_f16 and in parity16: the new mode holds the weights exactly (parity16 rounds them), generates the
    oracle's ids, and its hidden-state error is no larger than parity16's (exact weights, finer terms) and inside the f32 bound
    tests/test_gpu_parity16.py sets.  B = 4: two passes of the two-row GEMV; B = 6: the MFMA decode path on pairs.  At
    B = 1 the profile table shows the f16-pair kernels ran and none of the bf16 ones."""
    cfg = config_tiny()
    cfg = dataclasses.replace(cfg, llm=LlmConfig(vocab=1000, dim=4096, heads=32, layers=2, mlp=11008, max_seq=512))
    sd = f16_weights(cfg, seed=21, scale=0.02)
    sd32 = f32(sd)
    clip, sam, ids = make_inputs(cfg, B, seed=22, L=65)
    sizes, H, W = [(224, 224)] * B, [224] * B, [224] * B
    rig_seg(cfg, sd32, clip, sam, ids, sizes, (H, W))
    n_ref = min(B, 2)
    with torch.no_grad():
        ref = O.anyref_generate(sd32, cfg, clip[:n_ref], ids[:n_ref], sam[:n_ref], sizes[:n_ref], H[:n_ref], W[:n_ref],
                                max_new_tokens=6, eos=False)
    padded, mask = pad(ids)
    errs, inexact, scale = {}, {}, 1.0
    for mode in ("parity16", MODE):
        m = build(cfg, sd, mode, max_batch=B, max_seg=4)
        inexact[mode] = m.inexact_weights
        prof = mode == MODE and B == 1
        if prof:
            m.profile_enable(True)
        (out_ids, _, _), ex = m.generate(clip, padded, sam, sizes, H, W, max_new_tokens=6, attention_masks=mask,
                                         _return_extras=True)
        if prof:
            tags = m.profile_read()
            m.profile_enable(False)
            for t in ("gemm_sp16h_", "gemv_sp16h_x8", "gemv_sp16h_swiglu_x8", "gemv_sp16h_x24"):
                assert any(k.startswith(t) for k in tags), (t, sorted(tags))
            assert not any(k.startswith(("gemm_sp16_", "gemv_sp16_", "gemv_bf16", "gemm_bf16")) for k in tags), sorted(tags)
        worst = 0.0
        for b in range(n_ref):
            want_ids = ref["output_ids"][b]
            same = out_ids[b, : len(want_ids)].cpu().tolist() == want_ids.tolist()
            if mode == MODE:
                assert same, f"row {b}: greedy ids differ from the oracle"
            n = ref["hidden"][b].shape[0]
            Sp = len(ids[b]) + 255
            got, want = ex["hidden"][b, :n].cpu(), ref["hidden"][b]
            rows = n if same else Sp              # decode rows only along the same token path
            e = (got[:rows] - want[:rows]).abs().max().item()
            scale = max(scale, want.abs().max().item())
            print(f"[{mode} B={B}] row {b}: hidden max-abs-err {e:.3e} over {rows} rows (scale "
                  f"{want.abs().max().item():.2f}), ids identical: {same}")
            worst = max(worst, e)
        errs[mode] = worst
        del m
        gc.collect()
    print(f"[B={B}] hidden max-abs-err parity16 {errs['parity16']:.3e}, {MODE} {errs[MODE]:.3e}; inexact weights {inexact}")
    assert inexact[MODE] == 0 and inexact["parity16"] > 0, inexact
    assert errs[MODE] <= errs["parity16"], errs
    assert errs[MODE] < 2e-4 * scale, errs


def test_c2_full_size_vs_oracle():
    """C2 at full size (LLaMA-7B + CLIP ViT-L/14 + SAM-H at 1024^2, S = 320, 10 new tokens) on f16-rounded weights of the
    parity workload (init="fan_in"), 4 prompts, the first with masks, one oracle run shared by both handles.  Asserted for
    parity16_f16: ids identical on every prompt, mask logits within 1e-3 absolute (north_star's bar, as
    tests/test_gpu_c2_full.py asserts for parity16 on bf16-exact weights), no inexact weight, at most 17 GiB on the device.
    parity16 on the same fp16 weights runs beside it; its error is printed, not asserted."""
    cfg = config_7b()
    cfg.llm.max_seq = 512
    from anyref_amd.synth import synth_state_dict
    sd = synth_state_dict(cfg, seed=0, device="cuda", round_bf16=False, init="fan_in")
    sd = {k: v.half() if v.is_floating_point() else v for k, v in sd.items()}
    sd32 = {k: v.float().cpu() for k, v in sd.items()}
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(1, 3, 224, 224, generator=g)
    sam = torch.randn(1, 3, 1024, 1024, generator=g)
    NP = 4
    ids = [torch.cat([torch.tensor([1, -200]), torch.randint(3, 32000, (63,), generator=g)]) for _ in range(NP)]
    sizes, H, W = [(1024, 1024)], [1024], [1024]
    T_NEW = 10
    with torch.no_grad():
        img_feats = O.encode_images(sd32, cfg, clip)
        first = O.greedy_generate(sd32, cfg, O.splice_embeddings(sd32, cfg, ids[0], img_feats[0]), T_NEW, None)[0]
        cfg.seg_token_idx = int(first[2])
        img_emb = O.sam_image_encoder(sd32, cfg, sam)
        refs = []
        for i in range(NP):
            new_ids, hidden, _ = O.greedy_generate(sd32, cfg, O.splice_embeddings(sd32, cfg, ids[i], img_feats[0]), T_NEW, None)
            full = torch.cat([ids[i], torch.tensor(new_ids)])
            r = dict(output_ids=[full], hidden=[hidden], pred_masks=None)
            if i == 0:
                r["pred_masks"] = O.generate_tail(sd32, cfg, [full], [len(ids[i])], [hidden], None, sam, sizes, H, W,
                                                  image_embeddings=img_emb)["pred_masks"]
            refs.append(r)
    report = {}
    for mode in (MODE, "parity16"):
        m = build(cfg, sd, mode, max_batch=1, max_seg=4)
        rows = [compare_generate(m, refs[0], clip, ids[0], sam, sizes, H, W, T_NEW, sd32["lm_head.weight"], cfg.clip.n_patches)]
        herr, same = 0.0, []
        for i in range(NP):
            (out_ids, _, _), ex = m.generate(clip, ids[i][None], sam, sizes, H, W, max_new_tokens=T_NEW, _return_extras=True)
            want_ids, want = refs[i]["output_ids"][0], refs[i]["hidden"][0]
            s = out_ids[0, : len(want_ids)].cpu().tolist() == want_ids.tolist()
            same.append(s)
            n = want.shape[0] if s else len(ids[i]) + cfg.clip.n_patches - 1
            herr = max(herr, (ex["hidden"][0, :n].cpu() - want[:n]).abs().max().item() / max(1.0, want.abs().max().item()))
        report[mode] = dict(summarize(rows), ids_identical=same, hidden_rel_err=herr, inexact_weights=m.inexact_weights,
                            device_gib=round(m.device_bytes / GIB, 3))
        del m
        gc.collect()
        torch.cuda.empty_cache()
    print("C2_FULL_PARITY16_F16 " + json.dumps(report), flush=True)
    p, q = report[MODE], report["parity16"]
    print(f"C2 {MODE} mask logits: max-abs-err {p['mask_logit_max_abs_err']:.3e} (bar 1e-3), ids {p['ids_identical']}, "
          f"hidden rel {p['hidden_rel_err']:.3e}, {p['device_gib']} GiB; parity16 on the same fp16 weights (not asserted): "
          f"{q['mask_logit_max_abs_err']:.3e}, ids {q['ids_identical']}, hidden rel {q['hidden_rel_err']:.3e}, "
          f"inexact weights {q['inexact_weights']}")
    assert all(p["ids_identical"]), p
    assert p["ids_match_rate"] == 1.0, p
    assert p["mask_logit_max_abs_err"] <= MASK_TOL, p
    assert p["inexact_weights"] == 0, p
    assert p["device_gib"] <= 17.0, p


def test_from_pretrained_fp16_checkpoint(tmp_path):
    """an HF directory with fp16 safetensors shards through from_pretrained in the new mode: every weight held exactly, the
    oracle's ids; parity16 on the same directory reports the elements it rounded to bf16"""
    from safetensors.torch import save_file
    from anyref_amd.model import AnyRefForCausalLM
    cfg = config_tiny()
    sd = f16_weights(cfg, seed=5, scale=0.05)
    base = os.path.join(str(tmp_path), "AnyRef-fp16")
    os.makedirs(base)
    l = cfg.llm
    json.dump(dict(architectures=["LlavaLlamaForCausalLM"], hidden_size=l.dim, intermediate_size=l.mlp,
                   num_hidden_layers=l.layers, num_attention_heads=l.heads, vocab_size=l.vocab, rms_norm_eps=l.rms_eps,
                   bos_token_id=1, eos_token_id=2, pad_token_id=0), open(os.path.join(base, "config.json"), "w"))
    names = sorted(sd)
    shards = {"model-00001-of-00002.safetensors": names[: len(names) // 2],
              "model-00002-of-00002.safetensors": names[len(names) // 2:]}
    wm = {}
    for f, ks in shards.items():
        save_file({k: sd[k].contiguous() for k in ks}, os.path.join(base, f))
        wm.update({k: f for k in ks})
    json.dump(dict(metadata={}, weight_map=wm), open(os.path.join(base, "model.safetensors.index.json"), "w"))
    g = torch.Generator().manual_seed(11)
    clip = torch.randn(1, 3, 224, 224, generator=g)
    sam = torch.randn(1, 3, 224, 224, generator=g)
    ids = torch.cat([torch.tensor([1, -200]), torch.randint(3, 990, (12,), generator=g)])
    sizes, H, W = [(224, 224)], [224], [224]
    sd32 = f32(sd)
    ocfg = dataclasses.replace(cfg)
    with torch.no_grad():
        r0 = O.anyref_generate(sd32, ocfg, clip, [ids], sam, sizes, H, W, max_new_tokens=4, eos=False)
        ocfg.seg_token_idx = int(r0["output_ids"][0][-2])
        ref = O.anyref_generate(sd32, ocfg, clip, [ids], sam, sizes, H, W, max_new_tokens=5, eos=False)
    counts = {}
    for mode in (MODE, "parity16"):
        model = AnyRefForCausalLM.from_pretrained(base, torch_dtype=torch.float16, mode=mode, max_seg=4, max_seq=512,
                                                  seg_token_idx=ocfg.seg_token_idx, out_dim=cfg.out_dim)
        model.cfg.clip, model.cfg.sam = cfg.clip, cfg.sam         # the tiny towers (the directory carries their tensors)
        assert all(v.dtype == torch.float16 for v in model.host_state_dict().values() if v.is_floating_point())
        model = model.cuda()
        model.config.eos_token_id = None
        counts[mode] = model.inexact_weights
        if mode == MODE:
            out_ids, masks, _ = model.generate(clip, ids[None], sam, sizes, H, W, max_new_tokens=5)
            assert out_ids[0].cpu().tolist() == ref["output_ids"][0].tolist()
            assert masks[0] is not None and masks[0].shape == ref["pred_masks"][0].shape
            err = (masks[0].cpu() - ref["pred_masks"][0]).abs().max().item()
            print(f"from_pretrained fp16 directory [{MODE}]: mask max-abs-err {err:.3e}")
            assert err <= MASK_TOL
        del model
    print(f"from_pretrained fp16 directory: inexact weights {counts}")
    assert counts[MODE] == 0 and counts["parity16"] > 0, counts
