#!/usr/bin/env python3
"""A/B of the refine pass (anyref_refine_masks) at C2 (LLaMA-7B + CLIP ViT-L/14 + SAM-H at 1024^2, S = 320, 10
new tokens; tools/ab_mask_reports.py's weights and prompt plus `synth_prompt_weights`), on ONE handle per mode.

Cases, timed alternately, round after round (`--rounds` x `--steps` calls each, after `--warmup` calls per case):
  plain         the plain `generate` call with spatial prompts reserved (Python then keeps the low-res logits of every call)
  plain_unreserved  the same call after `set_spatial_prompts(0)`: what a handle that never heard of the feature runs, and what
                `--unchanged` measures on another build
  session       one query behind an open image session (the session is reopened, untimed, at the start of its turn: the plain
                call ends it)
  refine_box    `refine(0, 0, box, mask_input=True)` of the plain call's mask (the call itself untimed)
  refine_points `refine(0, 0, three points, multimask_output=True)`
  decode_text   `mask_decode` with the text prompt alone at n = 1 on a held embedding: the decoder pass as it was, the yardstick
                for what the two prompt kernels and the longer token rows add
Then, alone and on events over warm repeats: prompt_tokens_kernel (n = 1, 3 points + text, C = 256) and
mask_prompt_embed_kernel (n = 1, g = 64, C = 256), the latter against its 8 MB of key traffic.

`--unchanged` times the plain call alone, with nothing reserved, and needs nothing of the feature: with `--tree DIR` (a checkout
of another commit, built) it is the parent's side.  `--parent-json FILE` (repeatable) folds such runs' output into this one's,
with the comparison against `plain_unreserved`.  `--fold FILE` measures nothing: it adds the `--parent-json` runs to an earlier
output of this tool (parent / this / parent: the second parent run ends after this build's).

Prints ONE JSON line; the default run also writes it to `--out` (profiles/ab_refine_c2.json).

usage: python tools/ab_refine.py [--rounds 5] [--steps 10] [--warmup 3] [--modes perf] [--unchanged] [--tree DIR]
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
HW = 1024


def _stats(v):
    return dict(mean=round(statistics.mean(v), 3), median=round(statistics.median(v), 3), min=round(min(v), 3),
                max=round(max(v), 3), spread=round(max(v) - min(v), 3), rounds=[round(x, 3) for x in v])


def kernels_alone(torch):
    import ctypes as C
    from anyref_amd import _lib
    lib = _lib.load()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Cc, g, nt1 = 256, 64, 5
    r = lambda *s: torch.randn(*s, device="cuda")
    out_tokens, gauss, emb5, text, pts = r(nt1, Cc), r(2, Cc // 2), r(5, Cc), r(1, Cc), torch.rand(1, 3, 2, device="cuda") * 1023
    lab = torch.tensor([[1, 0, 1]], dtype=torch.int32, device="cuda")
    tokens = torch.empty(1, nt1 + 3 + 1 + 1, Cc, device="cuda")
    mask, emb, keys = r(1, 4 * g, 4 * g) * 4, r(g * g, Cc), torch.empty(1, g * g, Cc, device="cuda")
    w = [r(4, 1, 2, 2), r(4), r(4), r(4), r(16, 4, 2, 2) / 4, r(16), r(16), r(16), r(Cc, 16) / 4, r(Cc)]

    def ok(rc):
        assert rc == 0, lib.anyref_op_last_error().decode()
    fns = (("prompt_tokens", lambda: ok(lib.anyref_op_prompt_tokens(st, P(out_tokens), nt1, P(pts), P(lab), 3, None, P(text), P(gauss),
                                                                    P(emb5), 1, Cc, 1024, P(tokens), 0))),
           ("mask_prompt_embed", lambda: ok(lib.anyref_op_mask_prompt_embed(st, P(mask), P(emb), *[P(t) for t in w], 1, g, Cc, 4, 16,
                                                                            P(keys), 0))))
    us = {n: [] for n, _ in fns}
    for rnd in range(12):
        for name, f in (fns if rnd % 2 == 0 else fns[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                f()
            b.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / 20)
    row = {n: dict(us_median=round(statistics.median(v[2:]), 2), us_min=round(min(v[2:]), 2), us_max=round(max(v[2:]), 2))
           for n, v in us.items()}
    traffic = 2 * 4 * g * g * Cc + 4 * 16 * g * g
    row["mask_prompt_embed"]["bytes"] = traffic
    row["mask_prompt_embed"]["GB_per_s"] = round(traffic / row["mask_prompt_embed"]["us_median"] / 1e3, 1)
    row["note"] = "20 back-to-back launches between two events (warm: the operands sit in the Infinity Cache); us per launch"
    return row


def fold_parents(out, paths, unchanged=False):
    """the parent commit's --unchanged runs beside this build's plain call with nothing reserved"""
    parents = []
    for path in paths:
        with open(path) as f:
            parents.append(json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1]))
    if not parents:
        return
    out["parent_runs"] = parents
    for mode, res in out["modes"].items():
        means = [q["modes"][mode]["plain"]["ms"]["mean"] for q in parents if mode in q.get("modes", {})]
        rounds = [x for q in parents if mode in q.get("modes", {}) for x in q["modes"][mode]["plain"]["ms"]["rounds"]]
        key = "plain" if unchanged else "plain_unreserved"
        if means and key in res:
            t = res[key]["ms"]
            res["unreserved_against_parent"] = dict(
                this_mean_ms=t["mean"], this_rounds_ms=t["rounds"], parent_means_ms=means,
                parent_rounds_min_max_ms=[min(rounds), max(rounds)],
                within_the_spread_of_the_parents_rounds=min(rounds) <= t["mean"] <= max(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="calls per case and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="perf")
    ap.add_argument("--unchanged", action="store_true", help="the plain call alone (runs on a build without the feature)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose anyref_amd is measured")
    ap.add_argument("--parent-json", action="append", default=[], help="output of an --unchanged run of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fold", default=None, help="no measurement: add the --parent-json runs to this earlier output and rewrite it")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            out = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
        fold_parents(out, args.parent_json, out.get("unchanged", False))
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
        raise SystemExit("ab_refine: --modes takes a comma-separated list of " + ", ".join(KNOWN))
    if not torch.cuda.is_available():
        raise SystemExit("ab_refine: needs an MI355X (there is no CPU measurement)")
    dev = torch.device("cuda", 0)
    cfg = config_7b()
    cfg.llm.max_seq = 512
    sd = synth_state_dict(cfg, seed=0, device=dev, round_bf16=False)
    if not args.unchanged:
        from anyref_amd.synth import synth_prompt_weights
        sd.update({k: v.to(dev) for k, v in synth_prompt_weights(cfg, seed=0).items()})
    sd = {k: v.half() if v.is_floating_point() else v for k, v in sd.items()}
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(1, 3, 224, 224, generator=g).to(dev)
    sam = torch.randn(1, 3, 1024, 1024, generator=g).to(dev)
    prefix = torch.cat([torch.tensor([1]), torch.randint(3, 32000, (N_PRE - 2,), generator=g), torch.tensor([IMAGE_TOKEN_INDEX])])
    full = torch.cat([prefix, torch.randint(3, 32000, (N_SUF,), generator=g)])[None]
    L = full.shape[1]
    sizes, H, W = [(1024, 1024)], [HW], [HW]
    box = [200.0, 150.0, 800.0, 900.0]
    pts, lab = [[300.0, 300.0], [600.0, 500.0], [100.0, 900.0]], [1, 1, 0]

    result = {}
    for mode in modes:
        m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=1, max_seg=2)
        m.config.eos_token_id = None
        plain = lambda: m.generate(clip, full, sam, sizes, H, W, max_new_tokens=T_NEW)
        out_ids, _, _ = plain()
        m.set_seg_token_idx(int(out_ids[0, L + 2]))            # bench.py's rule: the id emitted at step 3 is [SEG]
        ref = plain()
        state = {}
        if args.unchanged:
            cases = {"plain": (lambda: None, plain)}
        else:
            m.set_spatial_prompts(8)
            got = plain()
            assert torch.equal(got[0], ref[0]) and all(torch.equal(a, b) for a, b in zip(got[1], ref[1])), \
                f"{mode}: the plain call with spatial prompts reserved differs"
            z = m.refine(0, 0)
            assert torch.equal(z["masks"][0], ref[1][0][0]), f"{mode}: refine without a prompt is not the call's mask"
            emb = m.sam_encode(sam)
            pred = torch.randn(1, cfg.out_dim, device=dev) * 0.5

            def open_session():
                state["sess"] = m.image_session(clip[0], sam[0], sizes[0], H[0], W[0], prefix)
            def reserved(then=lambda: None):
                def go():
                    if not m._sp_max:
                        m.set_spatial_prompts(8)
                    then()
                return go
            cases = {"plain": (reserved(), plain),
                     "plain_unreserved": (lambda: m.set_spatial_prompts(0), plain),
                     "session": (reserved(open_session), lambda: state["sess"].generate(full, max_new_tokens=T_NEW)),
                     "refine_box": (reserved(plain), lambda: m.refine(0, 0, box=box, mask_input=True)),
                     "refine_points": (reserved(plain), lambda: m.refine(0, 0, points=pts, labels=lab, multimask_output=True)),
                     "decode_text": (reserved(), lambda: m.mask_decode(emb[0], pred, sizes[0], (H[0], W[0])))}
        names = tuple(cases)
        for name in names:
            cases[name][0]()
            for _ in range(args.warmup):
                cases[name][1]()
        torch.cuda.synchronize()
        per = {name: [] for name in names}
        for r in range(args.rounds):
            for name in (names if r % 2 == 0 else names[::-1]):
                cases[name][0]()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    cases[name][1]()
                torch.cuda.synchronize()
                per[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        result[mode] = {name: dict(ms=_stats(per[name])) for name in names}
        if not args.unchanged:
            result[mode]["refine_below_plain_and_session_every_round"] = all(
                max(a, b) < min(p, s) for a, b, p, s in zip(per["refine_box"], per["refine_points"], per["plain"], per["session"]))
            result[mode]["refine_minus_decode_text_us"] = {
                k: round((statistics.mean(per[k]) - statistics.mean(per["decode_text"])) * 1e3, 1)
                for k in ("refine_box", "refine_points")}
        del m
        gc.collect()
        torch.cuda.empty_cache()
    out = dict(workload="c2 (7B + ViT-L + SAM-H 1024^2, S = 320, 10 new tokens), f16-rounded N(0, 0.02^2) weights, one handle per "
                        "mode with max_batch 1; host wall time per call, ms", tree=os.path.relpath(os.path.abspath(args.tree), ROOT),
               unchanged=args.unchanged, rounds=args.rounds, steps=args.steps, modes=result)
    if not args.unchanged:
        out["kernels_alone"] = kernels_alone(torch)
    fold_parents(out, args.parent_json, args.unchanged)
    line = json.dumps(out)
    print(line, flush=True)
    path = args.out or (None if args.unchanged else os.path.join(ROOT, "profiles", "ab_refine_c2.json"))
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
