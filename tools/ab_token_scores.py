#!/usr/bin/env python3
"""A/B of token scores (anyref_set_token_scores) at C2 (LLaMA-7B + CLIP ViT-L/14 + SAM-H at 1024^2, S = 320, 10
new tokens; tools/ab_session.py's weights and prompt), on ONE handle per mode.

Default run: the plain `generate` call with the switch off and on, the two timed alternately, round after round (`--rounds` x
`--steps` calls each, after `--warmup` calls per case).  Before the timing, untimed: the ids of the two settings must be equal,
and the scores of the answer are read once (they go into the JSON: this is the top-2 gap the project's notes on flipped ids
speak of).  Then, alone and on events over warm repeats: `token_scores_kernel` on [1, 32007] and [36, 32007] f32 logits and
`argmax_kernel` on the same rows -- same bytes, same grid, the yardstick for the new kernel.

The on - off difference per image is set beside its prediction: (decode steps + 1) launches of the kernel, each its stand-alone
time plus the 1.5 us launch boundary DESIGN.md §10 uses for this chip.

`--unchanged` times the switch-off call alone and needs nothing of the feature: with `--tree DIR` (a checkout of another
commit, built) it is the parent's side of "the call costs what it cost".  `--parent-json FILE` folds such a run's output into
this one's, with the comparison the README row quotes.

Prints ONE JSON line; the default run also writes it to `--out` (profiles/ab_token_scores_c2.json).

usage: python tools/ab_token_scores.py [--rounds 5] [--steps 10] [--warmup 3] [--modes perf] [--unchanged] [--tree DIR]
                                       [--parent-json FILE] [--out FILE]
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
T_NEW = 10
N_PRE, N_SUF = 36, 29
VOCAB = 32007
LAUNCH_BOUNDARY_US = 1.5


def kernels_alone(torch):
    """token_scores_kernel and argmax_kernel by themselves on the same rows: per round 20 launches of each between two events,
    the two alternated; us per launch (warm: the rows sit in L2, as behind the lm_head in a decode step)"""
    import ctypes as C
    from anyref_amd import _lib
    lib = _lib.load()
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for M in (1, 36):
        x = torch.randn(M, VOCAB, device="cuda") * 3.0
        lp, gap = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
        ids = torch.zeros(M, dtype=torch.int64, device="cuda")

        def scores():
            return lib.anyref_op_token_scores(st, P(x), M, VOCAB, VOCAB, None, P(lp), P(gap), None)

        def argmax():
            return lib.anyref_op_argmax(st, P(x), M, VOCAB, VOCAB, P(ids), None, None, 0, 0, 0, None, None, None)

        us = dict(token_scores=[], argmax=[])
        for r in range(12):
            pair = (("token_scores", scores), ("argmax", argmax))
            for name, f in (pair if r % 2 == 0 else pair[::-1]):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(20):
                    assert f() == 0, lib.anyref_op_last_error().decode()
                b.record()
                torch.cuda.synchronize()
                us[name].append(a.elapsed_time(b) * 1e3 / 20)
        row = {n: dict(us_median=round(statistics.median(v[2:]), 2), us_min=round(min(v[2:]), 2), us_max=round(max(v[2:]), 2))
               for n, v in us.items()}
        row["ratio_to_argmax"] = round(row["token_scores"]["us_median"] / row["argmax"]["us_median"], 3)
        out[f"{M}x{VOCAB}"] = row
    out["note"] = "20 back-to-back launches between two events: a launch's time includes its boundary to the next"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="calls per case and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="perf")
    ap.add_argument("--unchanged", action="store_true", help="the switch-off call alone (runs on a build without the feature)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose anyref_amd is measured")
    ap.add_argument("--parent-json", default=None, help="output of an --unchanged run of the parent commit, to compare with")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from anyref_amd.config import config_7b, IMAGE_TOKEN_INDEX
    from anyref_amd.model import AnyRefForCausalLM
    from anyref_amd.synth import synth_state_dict

    modes = tuple(args.modes.split(","))
    if any(m not in KNOWN for m in modes):
        raise SystemExit("ab_token_scores: --modes takes a comma-separated list of " + ", ".join(KNOWN))
    if not torch.cuda.is_available():
        raise SystemExit("ab_token_scores: needs an MI355X (there is no CPU measurement)")
    dev = torch.device("cuda", 0)
    cfg = config_7b()
    cfg.llm.max_seq = 512
    sd = synth_state_dict(cfg, seed=0, device=dev, round_bf16=False)
    sd = {k: v.half() if v.is_floating_point() else v for k, v in sd.items()}
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(1, 3, 224, 224, generator=g).to(dev)
    sam = torch.randn(1, 3, 1024, 1024, generator=g).to(dev)
    prefix = torch.cat([torch.tensor([1]), torch.randint(3, 32000, (N_PRE - 2,), generator=g), torch.tensor([IMAGE_TOKEN_INDEX])])
    full = torch.cat([prefix, torch.randint(3, 32000, (N_SUF,), generator=g)])[None]
    L = full.shape[1]
    sizes, H, W = [(1024, 1024)], [1024], [1024]
    cases = ("off",) if args.unchanged else ("off", "on")

    result = {}
    for mode in modes:
        m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=1, max_seg=2)
        m.config.eos_token_id = None
        plain = lambda: m.generate(clip, full, sam, sizes, H, W, max_new_tokens=T_NEW)
        out_ids, _, _ = plain()
        m.set_seg_token_idx(int(out_ids[0, L + 2]))            # bench.py's rule: the id emitted at step 3 is [SEG]
        answer = plain()[0][0, L:].tolist()
        extra = {}

        def prepare(case):
            if not args.unchanged:
                m.set_token_scores(case == "on")

        if not args.unchanged:                                 # untimed: same ids, and what the scores say about them
            prepare("on")
            got = plain()[0][0, L:].tolist()
            assert got == answer, f"{mode}: ids with the switch on differ: {got} vs {answer}"
            sc = m.last_token_scores()[0]
            assert len(sc["gap"]) == T_NEW
            extra = dict(answer=answer, logprob=[round(v, 4) for v in sc["logprob"].tolist()],
                         gap=[round(v, 5) for v in sc["gap"].tolist()], min_gap=round(min(sc["gap"].tolist()), 5))
        for case in cases:
            prepare(case)
            for _ in range(args.warmup):
                plain()
        torch.cuda.synchronize()
        per = {case: [] for case in cases}
        for r in range(args.rounds):
            for case in (cases if r % 2 == 0 else cases[::-1]):
                prepare(case)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    plain()
                torch.cuda.synchronize()
                per[case].append((time.perf_counter() - t0) * 1e3 / args.steps)
        result[mode] = {case: dict(ms=dict(mean=round(statistics.mean(per[case]), 3), median=round(statistics.median(per[case]), 3),
                                           min=round(min(per[case]), 3), max=round(max(per[case]), 3),
                                           spread=round(max(per[case]) - min(per[case]), 3), rounds=[round(x, 3) for x in per[case]]))
                        for case in cases}
        if not args.unchanged:
            result[mode]["scores_of_the_answer"] = extra
            result[mode]["on_minus_off_us"] = dict(
                mean=round((statistics.mean(per["on"]) - statistics.mean(per["off"])) * 1e3, 1),
                per_round=[round((a - b) * 1e3, 1) for a, b in zip(per["on"], per["off"])])
        del m
        gc.collect()
        torch.cuda.empty_cache()
    out = dict(workload="c2 (7B + ViT-L + SAM-H 1024^2, S = 320, 10 new tokens), f16-rounded N(0, 0.02^2) weights, one handle per "
                        "mode with max_batch 1; the plain generate call",
               tree=os.path.relpath(os.path.abspath(args.tree), ROOT), unchanged=args.unchanged, rounds=args.rounds,
               steps=args.steps, modes=result)
    if not args.unchanged:
        out["kernels_alone"] = k = kernels_alone(torch)
        one = k[f"1x{VOCAB}"]["token_scores"]["us_median"]
        for mode in modes:
            result[mode]["on_minus_off_us"]["predicted"] = round(T_NEW * (one + LAUNCH_BOUNDARY_US), 1)
            result[mode]["on_minus_off_us"]["predicted_from"] = (f"{T_NEW} launches (first token + {T_NEW - 1} decode steps) x "
                                                                 f"({one} us alone + {LAUNCH_BOUNDARY_US} us launch boundary)")
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
        out["parent"] = parent
        for mode in modes:
            if mode in parent.get("modes", {}):
                p, t = parent["modes"][mode]["off"]["ms"], result[mode]["off"]["ms"]
                result[mode]["off_against_parent"] = dict(
                    this_mean_ms=t["mean"], this_spread_ms=t["spread"], parent_mean_ms=p["mean"], parent_spread_ms=p["spread"],
                    difference_ms=round(t["mean"] - p["mean"], 3), within_parent_spread=abs(t["mean"] - p["mean"]) <= p["spread"])
    line = json.dumps(out)
    print(line, flush=True)
    path = args.out or (None if args.unchanged else os.path.join(ROOT, "profiles", "ab_token_scores_c2.json"))
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
