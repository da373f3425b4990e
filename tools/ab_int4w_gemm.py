#!/usr/bin/env python3
"""Timings of what the int4-operand GEMM changes in `perf_int4w`, for an A/B between two BUILDS of the library: run this script
once per build and round, alternately, each run a process of its own (`--tree DIR` imports anyref_amd from another checkout's
build).  One JSON line per run:

  prefill_ms   {mode: median}   generate(max_new_tokens = 1) at C2 (tools/ab_perf_f16.py's workload: 7B + ViT-L + SAM-H at
                                1024^2, S = 320, f16-rounded N(0, 0.02^2) weights, batch 1), `perf` beside `perf_int4w`
  image_ms     {mode: median}   the same call with 10 new tokens (the C2 headline)
  prefill_gemm_us {tag: [us per launch, launches]}   the GEMM launches of one profiled prefill call in `perf_int4w` (a build
                                that dequantises first runs that pass outside these tags)
  decode12     step_ms, bytes   four LLaMA layers at 7B widths under the tiny towers, B = 12 (the MFMA decode rows inside the
                                captured graph): (generate with 1 + T tokens - generate with 1 token) / T, and the algorithmic
                                bytes the profile books per decode step for the `_dec` GEMM launches (a build that
                                dequantises first books the bf16 image there; the dequantise pass itself has no tag: it
                                reads 0.52 and writes 2 bytes per element on top)

usage: python tools/ab_int4w_gemm.py [--tree DIR] [--steps 10] [--warmup 3] [--skip-7b]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--skip-7b", action="store_true", help="decode12 only")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

from anyref_amd.config import IMAGE_TOKEN_INDEX, LlmConfig, config_7b, config_tiny  # noqa: E402
from anyref_amd.model import AnyRefForCausalLM  # noqa: E402
from anyref_amd.synth import synth_state_dict  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def c2(dev):
    cfg = config_7b()
    cfg.llm.max_seq = 512
    sd = synth_state_dict(cfg, seed=0, device=dev, round_bf16=False)
    sd = {k: v.half() if v.is_floating_point() else v for k, v in sd.items()}
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(1, 3, 224, 224, generator=g).to(dev)
    sam = torch.randn(1, 3, 1024, 1024, generator=g).to(dev)
    ids = torch.cat([torch.tensor([1, IMAGE_TOKEN_INDEX]), torch.randint(3, 32000, (63,), generator=g)])[None]
    sizes, H, W = [(1024, 1024)], [1024], [1024]
    prefill, image, nbytes = {}, {}, {}
    for mode in ("perf", "perf_int4w"):
        m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=1, max_seg=2)
        m.config.eos_token_id = None
        out_ids, _, _ = m.generate(clip, ids, sam, sizes, H, W, max_new_tokens=10)
        m.set_seg_token_idx(int(out_ids[0, ids.shape[1] + 2]))     # bench.py's rule: the id emitted at step 3 is [SEG]
        prefill[mode] = round(timed(lambda: m.generate(clip, ids, sam, sizes, H, W, max_new_tokens=1), args.steps, args.warmup), 3)
        image[mode] = round(timed(lambda: m.generate(clip, ids, sam, sizes, H, W, max_new_tokens=10), args.steps, args.warmup), 3)
        nbytes[mode] = m.device_bytes
        if mode == "perf_int4w":
            m.profile_enable(True)
            m.generate(clip, ids, sam, sizes, H, W, max_new_tokens=1)
            prof = m.profile_read()
            m.profile_enable(False)
            gemm_us = {k: [round(v["ms"] * 1e3 / max(1, v["count"]), 2), int(v["count"])] for k, v in sorted(prof.items())
                       if k.startswith("gemm_bf16_") or k.startswith("splitk")}
        del m
    return dict(prefill_ms=prefill, image_ms=image, device_bytes=nbytes, prefill_gemm_us=gemm_us)


def decode12(dev, B=12, T=16):
    cfg = config_tiny()
    cfg = dataclasses.replace(cfg, llm=LlmConfig(vocab=1000, dim=4096, heads=32, layers=4, mlp=11008, max_seq=512))
    sd = synth_state_dict(cfg, seed=2, scale=0.02)
    sd = {k: v.to(dev) for k, v in sd.items()}
    g = torch.Generator().manual_seed(3)
    clip = torch.randn(B, 3, cfg.clip.image_size, cfg.clip.image_size, generator=g).to(dev)
    sam = torch.randn(B, 3, cfg.sam.img_size, cfg.sam.img_size, generator=g).to(dev)
    ids = torch.cat([torch.tensor([1, IMAGE_TOKEN_INDEX]), torch.randint(3, 900, (30,), generator=g)])[None].repeat(B, 1)
    S = cfg.sam.img_size
    sizes, H, W = [(S, S)] * B, [S] * B, [S] * B
    m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode="perf_int4w", max_batch=B, max_seg=2)
    m.config.eos_token_id = None
    m.set_seg_token_idx(cfg.llm.vocab - 1)

    def gen(n):
        return lambda: m.generate(clip, ids, sam, sizes, H, W, max_new_tokens=n)
    t1 = timed(gen(1), args.steps, args.warmup)
    tn = timed(gen(1 + T), args.steps, args.warmup)

    def booked(n):
        m.profile_enable(True)
        gen(n)()
        prof = m.profile_read()
        m.profile_enable(False)
        return {k: v for k, v in prof.items() if k.startswith("gemm_") and k.endswith("_dec")}
    p1, pn = booked(1), booked(1 + T)
    per_step = {k: (v["bytes"] - p1.get(k, {"bytes": 0.0})["bytes"]) / T for k, v in pn.items()}
    return dict(step_ms=round((tn - t1) / T, 4), bytes_per_step={k: int(v) for k, v in sorted(per_step.items())},
                bytes_per_step_total=int(sum(per_step.values())), layers=cfg.llm.layers, batch=B)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("ab_int4w_gemm: needs an MI355X (there is no CPU measurement)")
    dev = torch.device("cuda", 0)
    out = dict(tree=os.path.abspath(args.tree), steps=args.steps)
    out["decode12"] = decode12(dev)
    if not args.skip_7b:
        out.update(c2(dev))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
