#!/usr/bin/env python3
"""A/B of mask reports (anyref_set_mask_reports) at C2 (LLaMA-7B + CLIP ViT-L/14 + SAM-H at 1024^2, S = 320, 10
new tokens; tools/ab_token_scores.py's weights and prompt), on ONE handle per mode.

Default run: the plain `generate` call with the switch off, on (records only) and on with packed masks, timed alternately,
round after round (`--rounds` x `--steps` calls each, after `--warmup` calls per case).  Before the timing, untimed: ids and
masks of the three settings must be equal bit for bit, and the reports of the answer are read once and held to the rule
(anyref_amd/maskreport.py); they go into the JSON.  Then, alone and on events over warm repeats: `mask_report_kernel` (with its
clear and its box pass, as every launch has them) on [1, 1024, 1024] and [4, 1024, 1024] f32 logits, with and without packed
words, and `iou_counts_kernel` on the same logits -- it reads the same 4 MB per mask plus 1 MB of labels, the yardstick for the
new kernel.  Last: what the caller saves, the device-to-host copy of one 1024^2 f32 plane against its packed mask + record.

The on - off difference per image is set beside its prediction: one report launch per postprocess launch, each its stand-alone
time plus the 1.5 us launch boundary DESIGN.md §10 uses for this chip.  At batch 1 the early masks run on the side stream, under
the remaining decode steps: what of the prediction is hidden there does not show in the call.

`--unchanged` times the switch-off call alone and needs nothing of the feature: with `--tree DIR` (a checkout of another
commit, built) it is the parent's side of "the call costs what it cost".  `--parent-json FILE` (repeatable) folds such runs'
output into this one's, with the comparison the README row quotes.

Prints ONE JSON line; the default run also writes it to `--out` (profiles/ab_mask_reports_c2.json).

`--fold FILE` measures nothing: it adds the `--parent-json` runs to an earlier output of this tool (parent / this / parent: the
second parent run ends after this build's).

usage: python tools/ab_mask_reports.py [--rounds 5] [--steps 10] [--warmup 3] [--modes perf] [--unchanged] [--tree DIR]
                                       [--parent-json FILE ...] [--out FILE] [--fold FILE]
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
LAUNCH_BOUNDARY_US = 1.5
HW = 1024


def _timed(torch, fns, rounds=12, reps=20):
    """per round `reps` back-to-back launches of each function between two events, the functions alternated; us per launch"""
    us = {name: [] for name, _ in fns}
    for r in range(rounds):
        for name, f in (fns if r % 2 == 0 else fns[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / reps)
    return {n: dict(us_median=round(statistics.median(v[2:]), 2), us_min=round(min(v[2:]), 2), us_max=round(max(v[2:]), 2))
            for n, v in us.items()}


def kernels_alone(torch):
    """mask_report_kernel and iou_counts_kernel by themselves on the same logits (warm: 4 - 16 MB sit in the Infinity Cache, as
    behind the postprocess that wrote them)"""
    import ctypes as C
    from anyref_amd import _lib
    lib = _lib.load()
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for n in (1, 4):
        x = torch.randn(n, HW, HW, device="cuda") * 2.0
        tgt = (torch.rand(n, HW, HW, device="cuda") > 0.5).to(torch.uint8)
        rec = torch.zeros(n, 8, dtype=torch.int32, device="cuda")
        pk = torch.zeros(n, HW, HW // 32, dtype=torch.int32, device="cuda")
        counts = torch.zeros(n, 6, dtype=torch.int64, device="cuda")

        def ok(rc):
            assert rc == 0, lib.anyref_op_last_error().decode()

        fns = (("mask_report", lambda: ok(lib.anyref_op_mask_report(st, P(x), n, HW, HW, 1.0, P(rec), None))),
               ("mask_report_packed", lambda: ok(lib.anyref_op_mask_report(st, P(x), n, HW, HW, 1.0, P(rec), P(pk)))),
               ("iou_counts", lambda: ok(lib.anyref_op_iou_counts(st, P(x), P(tgt), n, HW * HW, P(counts)))))
        row = _timed(torch, fns)
        read = n * HW * HW * 4
        for name, extra in (("mask_report", 0), ("mask_report_packed", n * HW * HW // 8), ("iou_counts", n * HW * HW)):
            row[name]["bytes"] = read + extra
            row[name]["GB_per_s"] = round((read + extra) / row[name]["us_median"] / 1e3, 1)
        row["ratio_to_iou_counts"] = round(row["mask_report"]["us_median"] / row["iou_counts"]["us_median"], 3)
        row["ratio_packed_to_iou_counts"] = round(row["mask_report_packed"]["us_median"] / row["iou_counts"]["us_median"], 3)
        out[f"{n}x{HW}x{HW}"] = row
    out["note"] = ("20 back-to-back launches between two events: a launch's time includes its boundary to the next; a mask_report "
                   "launch is a clear of the records, the kernel and the box pass, an iou_counts launch a clear and the kernel")
    return out


def copies(torch):
    """what the caller saves: one 1024^2 f32 plane to pinned host memory, against its packed mask + record"""
    plane = torch.randn(HW, HW, device="cuda")
    small = torch.zeros(HW * HW // 32 + 8, dtype=torch.int32, device="cuda")
    h_plane = torch.empty(HW, HW, dtype=torch.float32).pin_memory()
    h_small = torch.empty(HW * HW // 32 + 8, dtype=torch.int32).pin_memory()
    row = _timed(torch, (("f32_plane", lambda: h_plane.copy_(plane, non_blocking=True)),
                         ("packed_and_record", lambda: h_small.copy_(small, non_blocking=True))), rounds=8, reps=10)
    row["f32_plane"]["bytes"], row["packed_and_record"]["bytes"] = HW * HW * 4, (HW * HW // 32 + 8) * 4
    row["ratio"] = round(row["f32_plane"]["us_median"] / row["packed_and_record"]["us_median"], 1)
    return row


def fold_parents(out, paths):
    """the parent commit's --unchanged runs beside this build's switch-off call"""
    parents = []
    for path in paths:
        with open(path) as f:
            parents.append(json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1]))
    out["parent_runs"] = parents
    for mode, res in out["modes"].items():
        means = [p["modes"][mode]["off"]["ms"]["mean"] for p in parents if mode in p.get("modes", {})]
        if means:
            t = res["off"]["ms"]
            lo, hi = min(means), max(means)
            res["off_against_parent"] = dict(
                this_mean_ms=t["mean"], this_spread_ms=t["spread"], parent_means_ms=means,
                within_the_parents_own_runs=lo <= t["mean"] <= hi,
                distance_outside_ms=round(max(lo - t["mean"], t["mean"] - hi, 0.0), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="calls per case and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="perf")
    ap.add_argument("--unchanged", action="store_true", help="the switch-off call alone (runs on a build without the feature)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose anyref_amd is measured")
    ap.add_argument("--parent-json", action="append", default=[], help="output of an --unchanged run of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fold", default=None, help="no measurement: add the --parent-json runs to this earlier output and rewrite it")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            out = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
        fold_parents(out, args.parent_json)
        line = json.dumps(out)
        print(line, flush=True)
        with open(args.out or args.fold, "w") as f:
            f.write(line + "\n")
        return
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from anyref_amd.config import config_7b, IMAGE_TOKEN_INDEX
    from anyref_amd.model import AnyRefForCausalLM
    from anyref_amd.synth import synth_state_dict

    modes = tuple(args.modes.split(","))
    if any(m not in KNOWN for m in modes):
        raise SystemExit("ab_mask_reports: --modes takes a comma-separated list of " + ", ".join(KNOWN))
    if not torch.cuda.is_available():
        raise SystemExit("ab_mask_reports: needs an MI355X (there is no CPU measurement)")
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
    sizes, H, W = [(1024, 1024)], [HW], [HW]
    cases = ("off",) if args.unchanged else ("off", "records", "packed")

    result = {}
    for mode in modes:
        m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=1, max_seg=2)
        m.config.eos_token_id = None
        plain = lambda: m.generate(clip, full, sam, sizes, H, W, max_new_tokens=T_NEW)
        out_ids, _, _ = plain()
        m.set_seg_token_idx(int(out_ids[0, L + 2]))            # bench.py's rule: the id emitted at step 3 is [SEG]
        ref = plain()
        answer = ref[0][0, L:].tolist()
        extra = {}

        def prepare(case):
            if not args.unchanged:
                m.set_mask_reports(case != "off", 1.0, packed=case == "packed")

        if not args.unchanged:                                 # untimed: same ids and masks, and the reports against the rule
            from anyref_amd.maskreport import mask_report_rule, stability
            for case in ("records", "packed"):
                prepare(case)
                got = plain()
                assert got[0][0, L:].tolist() == answer, f"{mode}: ids with the switch on differ"
                assert all(torch.equal(a, b) for a, b in zip(got[1], ref[1])), f"{mode}: masks with the switch on differ"
                rep = m.last_mask_reports()[0]
                rec, words = mask_report_rule(got[1][0].cpu().numpy(), 1.0)
                assert rep["area"].tolist() == rec[:, 0].tolist() and rep["box"].tolist() == rec[:, 4:].tolist(), f"{mode}: records"
                assert rep["area_hi"].tolist() == rec[:, 1].tolist() and rep["area_lo"].tolist() == rec[:, 2].tolist()
                if case == "packed":
                    assert (rep["packed"].cpu().numpy().view("uint32") == words).all(), f"{mode}: packed words"
            extra = dict(answer=answer, masks=len(rep["area"]), early_masks=int(m.early_masks_done), area=rep["area"].tolist(),
                         box=rep["box"].tolist(), stability=[round(float(v), 5) for v in stability(rec)],
                         nonfinite=rep["nonfinite"].tolist())
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
            result[mode]["reports_of_the_answer"] = extra
            for case in ("records", "packed"):
                result[mode][f"{case}_minus_off_us"] = dict(
                    mean=round((statistics.mean(per[case]) - statistics.mean(per["off"])) * 1e3, 1),
                    per_round=[round((a - b) * 1e3, 1) for a, b in zip(per[case], per["off"])])
        del m
        gc.collect()
        torch.cuda.empty_cache()
    out = dict(workload="c2 (7B + ViT-L + SAM-H 1024^2, S = 320, 10 new tokens), f16-rounded N(0, 0.02^2) weights, one handle per "
                        "mode with max_batch 1; the plain generate call",
               tree=os.path.relpath(os.path.abspath(args.tree), ROOT), unchanged=args.unchanged, rounds=args.rounds,
               steps=args.steps, modes=result)
    if not args.unchanged:
        out["kernels_alone"] = k = kernels_alone(torch)
        out["device_to_host"] = copies(torch)
        one = k[f"1x{HW}x{HW}"]
        for mode in modes:
            n_masks = result[mode]["reports_of_the_answer"]["masks"]
            for case, key in (("records", "mask_report"), ("packed", "mask_report_packed")):
                us = one[key]["us_median"]
                result[mode][f"{case}_minus_off_us"]["predicted"] = round(n_masks * (us + LAUNCH_BOUNDARY_US), 1)
                result[mode][f"{case}_minus_off_us"]["predicted_from"] = (
                    f"{n_masks} launches (one per mask: each [SEG] is decoded by a postprocess of its own) x ({us} us alone + "
                    f"{LAUNCH_BOUNDARY_US} us launch boundary); {result[mode]['reports_of_the_answer']['early_masks']} of them on "
                    "the side stream under the decode steps")
    if args.parent_json:
        fold_parents(out, args.parent_json)
    line = json.dumps(out)
    print(line, flush=True)
    path = args.out or (None if args.unchanged else os.path.join(ROOT, "profiles", "ab_mask_reports_c2.json"))
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
