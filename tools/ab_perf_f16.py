#!/usr/bin/env python3
"""A/B of ANYREF_MODE_PERF_F16 against the bf16 perf mode at C2 (LLaMA-7B + CLIP ViT-L/14 + SAM-H at 1024^2, one image, S = 320
prompt, 10 new tokens) on the SAME weights: bench.py's workload (every matrix N(0, 0.02^2)) rounded once to
f16, so that neither handle is favoured by the weights it was given.

Both handles live in one process and are timed alternately, round after round (`--rounds` x `--steps` generate calls each,
after `--warmup` calls per handle), so that clock and neighbour drift fall on both alike.  Then, untimed, one profiled call
per handle gives the per-tag averages of the decode GEMVs and the decode attention.  Prints ONE JSON line:
  {"ms_per_image": {mode: {median, min, max, rounds: [...]}}, "device_bytes": {mode: n}, "inexact_weights": {mode: n},
   "tags": {mode: {tag: us per launch}}, "f16_over_bf16": {median image ratio, per GEMV tag pair ratio}}

`--modes A,B` alternates any two modes the same way (B over A), e.g. `--modes parity16,parity16_f16`: the ratio keys are then
named "<B>_over_<A>" and the GEMV tags are paired through the modes' type tokens (sp16 / sp16h / bf16 / f16 / f32).

usage: python tools/ab_perf_f16.py [--rounds 5] [--steps 20] [--warmup 3] [--modes perf,perf_f16]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from anyref_amd.config import config_7b, IMAGE_TOKEN_INDEX  # noqa: E402
from anyref_amd.model import AnyRefForCausalLM  # noqa: E402
from anyref_amd.synth import synth_state_dict  # noqa: E402

MODES = ("perf", "perf_f16")
TOKEN = {"parity": "f32", "perf": "bf16", "perf_fp8w": "fp8w", "perf_f16": "f16", "parity16": "sp16", "parity16_f16": "sp16h", "perf_int4w": "int4w"}
T_NEW = 10


def main():
    global MODES
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="generate calls per handle and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default=",".join(MODES), help="two mode names, A,B: B is reported over A")
    args = ap.parse_args()
    MODES = tuple(args.modes.split(","))
    if len(MODES) != 2 or any(m not in TOKEN for m in MODES):
        raise SystemExit("ab_perf_f16: --modes takes two of " + ", ".join(TOKEN))
    A, B = MODES
    if not torch.cuda.is_available():
        raise SystemExit("ab_perf_f16: needs an MI355X (there is no CPU measurement)")
    dev = torch.device("cuda", 0)
    cfg = config_7b()
    cfg.llm.max_seq = 512
    sd = synth_state_dict(cfg, seed=0, device=dev, round_bf16=False)
    sd = {k: v.half() if v.is_floating_point() else v for k, v in sd.items()}
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(1, 3, 224, 224, generator=g).to(dev)
    sam = torch.randn(1, 3, 1024, 1024, generator=g).to(dev)
    ids = torch.cat([torch.tensor([1, IMAGE_TOKEN_INDEX]), torch.randint(3, 32000, (63,), generator=g)])[None]
    sizes, H, W = [(1024, 1024)], [1024], [1024]

    models = {}
    for mode in MODES:
        m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=1, max_seg=2)
        m.config.eos_token_id = None
        out_ids, _, _ = m.generate(clip, ids, sam, sizes, H, W, max_new_tokens=T_NEW)
        m.set_seg_token_idx(int(out_ids[0, ids.shape[1] + 2]))     # bench.py's rule: the id emitted at step 3 is [SEG]
        models[mode] = m
    del sd

    def call(m):
        m.generate(clip, ids, sam, sizes, H, W, max_new_tokens=T_NEW)

    for mode in MODES:
        for _ in range(args.warmup):
            call(models[mode])
    torch.cuda.synchronize()
    per = {mode: [] for mode in MODES}
    for r in range(args.rounds):
        order = MODES if r % 2 == 0 else MODES[::-1]
        for mode in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call(models[mode])
            torch.cuda.synchronize()
            per[mode].append((time.perf_counter() - t0) * 1e3 / args.steps)

    tags = {}
    for mode in MODES:
        m = models[mode]
        m.profile_enable(True)
        call(m)
        prof = m.profile_read()
        m.profile_enable(False)
        tags[mode] = {k: round(v["ms"] * 1e3 / max(1, v["count"]), 2) for k, v in sorted(prof.items())
                      if k.startswith(("gemv_", "decode_attn_"))}
    ratio_tags = {}
    for k, v in tags[B].items():
        kb = k.replace("_" + TOKEN[B], "_" + TOKEN[A])
        if kb in tags[A] and tags[A][kb] > 0:
            ratio_tags[f"{k}/{kb}"] = round(v / tags[A][kb], 4)
    med = {mode: statistics.median(per[mode]) for mode in MODES}
    out = dict(
        workload="c2 (7B + ViT-L + SAM-H 1024^2, S 320, 10 new tokens), f16-rounded N(0, 0.02^2) weights, batch 1",
        rounds=args.rounds, steps=args.steps,
        ms_per_image={mode: dict(median=round(med[mode], 3), min=round(min(per[mode]), 3), max=round(max(per[mode]), 3),
                                 rounds=[round(x, 3) for x in per[mode]]) for mode in MODES},
        device_bytes={mode: models[mode].device_bytes for mode in MODES},
        inexact_weights={mode: models[mode].inexact_weights for mode in MODES},
        tags_us=tags,
        **{("f16_over_bf16" if MODES == ("perf", "perf_f16") else f"{B}_over_{A}"): dict(image=round(med[B] / med[A], 4), tags=ratio_tags)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
