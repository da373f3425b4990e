#!/usr/bin/env python3
"""A/B of adapter hot-swap (anyref_adapter_apply / anyref_update_weight) against the only way there was: a handle
rebuild.  C2 widths (LLaMA-7B + CLIP ViT-L/14 + SAM-H at 1024^2; tools/ab_session.py's weights), `adapters="qv"`, two rank-8
adapters X and Y on q_proj / v_proj of every layer, each carrying train.py's `modules_to_save` set (embed_tokens, lm_head,
text_hidden_fcs, the mask decoder's mask_tokens / output_upscaling / output_hypernetworks_mlps, audio_projector when built).

One handle per mode, `--rounds` rounds alternated in one process.  Per round:
  swap_x / swap_y   `set_adapter("X")` / `set_adapter("Y")`: host clock around the call, ended by a device synchronise
  merge_ms          `last_apply_ms` of those calls: the merge launches alone (a hipEvent pair)
  merge_tbps        the merge's algorithmic bytes, (4 + sizeof(W)) N K per target, over merge_ms; against the 5.8 - 5.9 TB/s the decode
                    GEMV reaches alone (a ratio is reported, no threshold)
  rebuild           a second handle built from the host state dict (`from_state_dict`: anyref_create + every set_weight +
                    finalize), disk reads excluded, then dropped.  The base values are used: the cost does not depend on them.
  gen_before / gen_after   `generate` (S = 320, 10 new tokens) on the handle before the round's first swap and after its last
The swap must be below the rebuild in every round (`swap_below_rebuild_in_every_round`).

Prints ONE JSON line.

usage: python tools/ab_adapter.py [--rounds 5] [--modes perf,perf_int4w,parity16] [--no-rebuild]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = ("parity", "perf", "perf_fp8w", "perf_f16", "parity16", "parity16_f16", "perf_int4w")
W_BYTES = dict(parity=4, perf=2, perf_f16=2, parity16=2, parity16_f16=2, perf_fp8w=1.0, perf_int4w=0.5 + 2 / 128)
GEMV_TBPS = 5.85
T_NEW, RANK, ALPHA = 10, 8, 16


def synth_adapter(torch, cfg, sd, seed, audio):
    """(pairs, saved) in checkpoint.read_adapter's terms, on the host: N(0, 0.05^2) pairs, N(0, 0.02^2) saved tensors in fp16"""
    g = torch.Generator().manual_seed(seed)
    H = cfg.llm.dim
    pairs = {f"model.layers.{i}.self_attn.{p}": (torch.randn(RANK, H, generator=g) * 0.05, torch.randn(H, RANK, generator=g) * 0.05)
             for i in range(cfg.llm.layers) for p in ("q_proj", "v_proj")}
    md = "model.visual_model.mask_decoder."
    names = [k for k in sd if k in ("model.embed_tokens.weight", "lm_head.weight") or k.startswith("model.text_hidden_fcs.")
             or k.startswith((md + "mask_tokens.", md + "output_upscaling.", md + "output_hypernetworks_mlps."))
             or (audio and k.startswith("model.audio_projector."))]
    saved = {k: (torch.randn(*sd[k].shape, generator=g) * 0.02).half() for k in names}
    return pairs, saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default="perf,perf_int4w,parity16")
    ap.add_argument("--no-rebuild", action="store_true", help="skip the rebuild side (swap times only)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from anyref_amd.config import config_7b, IMAGE_TOKEN_INDEX
    from anyref_amd.model import AnyRefForCausalLM
    from anyref_amd.synth import synth_state_dict

    modes = tuple(args.modes.split(","))
    if any(m not in KNOWN for m in modes):
        raise SystemExit("ab_adapter: --modes takes a comma-separated list of " + ", ".join(KNOWN))
    if not torch.cuda.is_available():
        raise SystemExit("ab_adapter: needs an MI355X (there is no CPU measurement)")
    dev = torch.device("cuda", 0)
    cfg = config_7b()
    cfg.llm.max_seq = 512
    sd = synth_state_dict(cfg, seed=0, device=dev, round_bf16=False)
    sd = {k: (v.half() if v.is_floating_point() else v).cpu() for k, v in sd.items()}     # the host state dict a caller holds
    audio = any(k.startswith("model.audio_projector.") for k in sd)
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(1, 3, 224, 224, generator=g).to(dev)
    sam = torch.randn(1, 3, 1024, 1024, generator=g).to(dev)
    full = torch.cat([torch.tensor([1]), torch.randint(3, 32000, (34,), generator=g), torch.tensor([IMAGE_TOKEN_INDEX]),
                      torch.randint(3, 32000, (29,), generator=g)])[None]
    sizes, H, W = [(1024, 1024)], [1024], [1024]
    adapters = {n: synth_adapter(torch, cfg, sd, seed, audio) for n, seed in (("X", 11), ("Y", 12))}
    scaling = ALPHA / RANK
    l = cfg.llm
    n_targets = 2 * l.layers

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    result = {}
    for mode in modes:
        plain = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=1, max_seg=2)
        plain_bytes = plain.device_bytes
        del plain
        gc.collect()
        m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=1, max_seg=2, adapters="qv")
        m.config.eos_token_id = None
        extra_bytes = m.device_bytes - plain_bytes
        for n, (pairs, saved) in adapters.items():
            m.add_adapter(n, pairs, saved, scaling)
        gen = lambda: m.generate(clip, full, sam, sizes, H, W, max_new_tokens=T_NEW)
        for _ in range(3):
            gen()
        m.set_adapter("X")
        m.set_adapter(None)                                    # warm: both directions once
        per = dict(swap_x=[], swap_y=[], merge_ms=[], rebuild=[], gen_before=[], gen_after=[])
        for r in range(args.rounds):
            per["gen_before"].append(statistics.median(timed(gen) for _ in range(3)))
            order = ("X", "Y") if r % 2 == 0 else ("Y", "X")
            for n in order:
                per["swap_" + n.lower()].append(timed(lambda: m.set_adapter(n)))
                per["merge_ms"].append(m.adapter_stats()["last_apply_ms"])
            per["gen_after"].append(statistics.median(timed(gen) for _ in range(3)))
            if not args.no_rebuild:
                box = []
                per["rebuild"].append(timed(lambda: box.append(AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=1,
                                                                                                max_seg=2))))
                del box
                gc.collect()
                torch.cuda.empty_cache()
        merge_bytes = n_targets * (4 + W_BYTES[mode]) * l.dim * l.dim
        med = {k: statistics.median(v) for k, v in per.items() if v}
        tbps = merge_bytes / (med["merge_ms"] * 1e-3) / 1e12
        swaps = per["swap_x"] + per["swap_y"]
        spread = max(per["gen_before"]) - min(per["gen_before"])
        result[mode] = dict(
            {k: dict(median=round(med[k], 3), min=round(min(v), 3), max=round(max(v), 3), rounds=[round(x, 3) for x in v])
             for k, v in per.items() if v},
            merge_algorithmic_bytes=int(merge_bytes), merge_tbps=round(tbps, 3), merge_over_gemv_tbps=round(tbps / GEMV_TBPS, 3),
            reservation_extra_device_bytes=int(extra_bytes), inexact_after=m.adapter_stats()["inexact"],
            gen_after_minus_before_ms=round(med["gen_after"] - med["gen_before"], 3), gen_before_spread_ms=round(spread, 3),
            gen_agrees_within_spread=abs(med["gen_after"] - med["gen_before"]) <= spread,
            **({} if args.no_rebuild else dict(
                rebuild_over_swap=round(med["rebuild"] / statistics.median(swaps), 1),
                swap_below_rebuild_in_every_round=max(swaps) < min(per["rebuild"]))))
        if not args.no_rebuild:
            assert result[mode]["swap_below_rebuild_in_every_round"], result[mode]
        del m
        gc.collect()
        torch.cuda.empty_cache()
    print(json.dumps(dict(
        workload="c2 widths (7B + ViT-L + SAM-H 1024^2, S 320, 10 new tokens), f16 N(0, 0.02^2) weights from a HOST state dict; "
                 f"adapters: rank {RANK} on q_proj / v_proj of {l.layers} layers + modules_to_save, lora_A / lora_B on the device, "
                 "saved tensors in pinned host memory",
        rounds=args.rounds, gemv_alone_tbps=GEMV_TBPS, modes=result)), flush=True)


if __name__ == "__main__":
    main()
