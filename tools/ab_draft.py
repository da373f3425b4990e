#!/usr/bin/env python3
"""A/B of the draft-verified greedy decode (anyref_set_draft) against the plain loop at C2 (LLaMA-7B + CLIP
ViT-L/14 + SAM-H at 1024^2, one image, S = 320 prompt, 10 new tokens; bench.py's weights, every matrix N(0, 0.02^2), rounded
once to f16 as tools/ab_perf_f16.py does), on ONE handle per mode.

Per mode the cases are timed alternately, round after round (`--rounds` x `--steps` generate calls each, after `--warmup` calls
per case), so that clock and neighbour drift fall on all alike:
  plain   no draft: the loop as it always ran (the baseline; compare with tools/ab_perf_f16.py --modes perf,perf on the parent)
  full    the plain answer as the draft: 9 tokens offered at 10 new tokens, all accepted, no decode step
  half    that draft corrupted at index 4: 4 accepted, 5 decode steps behind the pass
  wrong1  corrupted at index 1: one pass buys one token -- the price of a wrong guess
  wrong0  corrupted at index 0: the first token already differs, the pass is skipped
Before the timing, untimed, every case's output is checked against the plain call: identical ids in parity16; in the 16-bit
modes (ids not pinned) the hidden rows along the common prefix within the mode's bound (2.5 % of their scale).

`--rephrase W` (W > 0): the same with rephrase_weight = W, the [SEG] at the first answer index >= 2 whose id is new
(a span that is not empty), `set_rephrase_paths` on for the five cases, and one more case, `plain_off`: the plain call with the
switch off (today's behaviour, where a draft would be ignored), alternated with the others.

Prints ONE JSON line: {"modes": {mode: {case: {ms_per_image: {median, min, max, rounds}, offered, accepted, decode_steps,
verify_passes, over_plain, faster_than_plain_in_every_round}}}, ...}

usage: python tools/ab_draft.py [--rounds 5] [--steps 10] [--warmup 3] [--modes perf,perf_int4w,parity16] [--rephrase W]
"""
import argparse
import gc
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

KNOWN = ("parity", "perf", "perf_fp8w", "perf_f16", "parity16", "parity16_f16", "perf_int4w")
PINNED = ("parity", "parity16", "parity16_f16")       # modes whose greedy ids the project pins
HIDDEN_REL = 0.025                                    # tests/test_gpu_e2e.py PERF_HIDDEN_REL_7B
T_NEW = 10
CASES = ("plain", "full", "half", "wrong1", "wrong0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="generate calls per case and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="perf")
    ap.add_argument("--rephrase", type=float, default=0.0, help="rephrase_weight; > 0: the switch on, and the case plain_off")
    args = ap.parse_args()
    reph = args.rephrase > 0
    cases = CASES + ("plain_off",) if reph else CASES
    modes = tuple(args.modes.split(","))
    if any(m not in KNOWN for m in modes):
        raise SystemExit("ab_draft: --modes takes a comma-separated list of " + ", ".join(KNOWN))
    if not torch.cuda.is_available():
        raise SystemExit("ab_draft: needs an MI355X (there is no CPU measurement)")
    dev = torch.device("cuda", 0)
    cfg = config_7b()
    cfg.llm.max_seq = 512
    if reph:
        cfg.rephrase_weight = args.rephrase
    sd = synth_state_dict(cfg, seed=0, device=dev, round_bf16=False)
    sd = {k: v.half() if v.is_floating_point() else v for k, v in sd.items()}
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(1, 3, 224, 224, generator=g).to(dev)
    sam = torch.randn(1, 3, 1024, 1024, generator=g).to(dev)
    ids = torch.cat([torch.tensor([1, IMAGE_TOKEN_INDEX]), torch.randint(3, 32000, (63,), generator=g)])[None]
    L = ids.shape[1]
    sizes, H, W = [(1024, 1024)], [1024], [1024]
    V = cfg.llm.vocab

    def run(m, draft, extras=False, case=None):
        if reph:
            m.set_rephrase_paths(case != "plain_off")
        return m.generate(clip, ids, sam, sizes, H, W, max_new_tokens=T_NEW, _return_extras=extras, draft_ids=draft)

    result = {}
    for mode in modes:
        m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=1, max_seg=2)
        m.config.eos_token_id = None
        out_ids, _, _ = run(m, None)
        seg_at = 2                                             # bench.py's rule: the id emitted at step 3 is [SEG]
        if reph:                                               # ... or the first later id that is new: a span that is not empty
            a0, old = out_ids[0, L:].tolist(), set(ids[0].tolist())
            seg_at = next((i for i in range(2, T_NEW) if a0[i] not in old and a0[i] not in a0[:i]), 2)
        m.set_seg_token_idx(int(out_ids[0, L + seg_at]))
        (out_ids, _, _), ex0 = run(m, None, True)
        answer = out_ids[0, L:].tolist()

        def wrong(at):
            d = answer[:T_NEW - 1]
            d[at] = (d[at] + 1) % V
            return [d]

        drafts = dict(plain=None, full=[answer[:T_NEW - 1]], half=wrong(4), wrong1=wrong(1), wrong0=wrong(0), plain_off=None)
        slen = L + m.n_img - 1
        stats, checks = {}, {}
        for case in cases:                                     # untimed: counters and outputs
            (o, _, _), ex = run(m, drafts[case], True, case)
            got = o[0, L:].tolist()
            stats[case] = dict(offered=int(ex["draft_offered"][0]), accepted=int(ex["draft_accepted"][0]),
                               decode_steps=ex["decode_steps"], verify_passes=ex["verify_passes"])
            same = got == answer
            common = next((i for i, (a, b) in enumerate(zip(got, answer)) if a != b), T_NEW)
            n = slen + max(common - 1, 0)                      # hidden rows computed along the common token prefix
            scale = ex0["hidden"][0, :n].abs().max().item()
            herr = (ex["hidden"][0, :n] - ex0["hidden"][0, :n]).abs().max().item()
            checks[case] = dict(ids_equal_plain=same, hidden_rows=n, hidden_err=herr, hidden_scale=scale)
            if mode in PINNED:
                assert same, f"{mode} / {case}: ids differ from the plain call: {got} vs {answer}"
            assert herr <= HIDDEN_REL * scale, f"{mode} / {case}: hidden err {herr} on a scale of {scale}"
        for case in cases:
            for _ in range(args.warmup):
                run(m, drafts[case], case=case)
        torch.cuda.synchronize()
        per = {case: [] for case in cases}
        for r in range(args.rounds):
            for case in (cases if r % 2 == 0 else cases[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run(m, drafts[case], case=case)
                torch.cuda.synchronize()
                per[case].append((time.perf_counter() - t0) * 1e3 / args.steps)
        med = {case: statistics.median(per[case]) for case in cases}
        result[mode] = {case: dict(
            ms_per_image=dict(median=round(med[case], 3), min=round(min(per[case]), 3), max=round(max(per[case]), 3),
                              rounds=[round(x, 3) for x in per[case]]),
            over_plain=round(med[case] / med["plain"], 4),
            faster_than_plain_in_every_round=all(a < b for a, b in zip(per[case], per["plain"])),
            **stats[case], check=checks[case]) for case in cases}
        if reph:
            result[mode]["first_seg_span"] = answer.index(answer[seg_at])
            result[mode]["plain_not_above_plain_off"] = med["plain"] <= med["plain_off"]
        del m
        gc.collect()
        torch.cuda.empty_cache()
    print(json.dumps(dict(
        workload="c2 (7B + ViT-L + SAM-H 1024^2, S 320, 10 new tokens), f16-rounded N(0, 0.02^2) weights, batch 1",
        rounds=args.rounds, steps=args.steps, **(dict(rephrase_weight=args.rephrase) if reph else {}), modes=result)), flush=True)


if __name__ == "__main__":
    main()
