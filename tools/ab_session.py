#!/usr/bin/env python3
"""A/B of image sessions (anyref_session_open / anyref_session_generate) against the plain call at C2 (LLaMA-7B +
CLIP ViT-L/14 + SAM-H at 1024^2, 10 new tokens; tools/ab_draft.py's weights), on ONE handle per mode (max_batch 4).

The prompt is `system + image` (36 ids: P = 291 spliced prefix rows) followed by a question of 29 ids: S = 320 as in bench.py.
Per mode the cases are timed alternately, round after round (`--rounds` x `--steps` calls each, after `--warmup` calls per case):
  plain     (a) `generate` on the full prompt: what every query costs today
  open      (b) `image_session(...)` alone: CLIP tower, SAM encoder, prefill of the prefix
  query     (c) one `sess.generate` of one question on an open session
  query4    (d) one `sess.generate` of four questions, reported PER QUERY (the call's time / 4)
  drafted   (e) (c) with the plain answer as the draft (9 tokens offered)
Before the timing, untimed, the session's answer is checked against the plain call's: identical ids in parity16; in the 16-bit
modes (ids not pinned) the prompt's hidden rows within the mode's bound (2.5 % of their scale).

`--rephrase W` (W > 0) runs the same workload with rephrase_weight = W, the [SEG] a few tokens into the answer (the
first answer index >= 2 whose id is new, so the rephrased span is not empty), and these cases instead, the switch
(`set_rephrase_paths`) set per case on the one handle:
  plain          (a) plain call, switch off: today's behaviour, the baseline
  plain_on       (b) plain call, switch on
  query          (c) one session query            query4  (d) four queries in one call, per query
  drafted_plain  (e) plain call with the answer as the draft       drafted  (f) (c) with that draft
and times the tail alone at the C2 shape (e0 = 325, 32 heads, hd 128, span 9, bf16 cache): the per-image chain
(anyref_op_rephrase_chain) against the fused pair (anyref_op_seg_rephrase), on events, alternated.

`--plain-only` times (a) alone and needs nothing of the feature: with `--tree DIR` (a checkout of another commit, built) it is
the parent's side of "the plain call costs what it cost".

Prints ONE JSON line: {"modes": {mode: {case: {ms: {median, min, max, rounds}, ...}, query_below_plain_in_every_round}}, ...}

usage: python tools/ab_session.py [--rounds 5] [--steps 10] [--warmup 3] [--modes perf,perf_int4w,parity16] [--plain-only] [--tree DIR]
                                [--rephrase W]
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
PINNED = ("parity", "parity16", "parity16_f16")       # modes whose greedy ids the project pins
HIDDEN_REL = 0.025                                    # tests/test_gpu_e2e.py PERF_HIDDEN_REL_7B
T_NEW = 10
N_PRE, N_SUF, Q4 = 36, 29, 4


def broadcast_alone(torch, cfg, P):
    """the prefix broadcast kernel by itself (anyref_op_kv_broadcast) on buffers of the 16-bit modes' cache shape at max_batch 4:
    row 0's P positions of every layer of K and V to rows 1 - 3, between two events"""
    import ctypes as C
    from anyref_amd import _lib
    lib = _lib.load()
    l = cfg.llm
    k = torch.zeros(l.layers, Q4, l.max_seq, l.dim, dtype=torch.bfloat16, device="cuda")
    v = torch.zeros_like(k)
    ms = []
    for _ in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = lib.anyref_op_kv_broadcast(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(k.data_ptr()),
                                        C.c_void_p(v.data_ptr()), l.layers, Q4, l.max_seq, l.dim, 2, P, 1, Q4)
        e1.record()
        assert rc == 0, lib.anyref_op_last_error().decode()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[2:]
    moved = 2 * l.layers * P * l.dim * 2 * Q4                 # read once, stored three times
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), launches=1,
                bytes_read_and_written=moved, gb_per_s=round(moved / statistics.median(ms) / 1e6, 1))


def tail_alone(torch):
    """the rephrase tail by itself at the C2 shape: one item, query row 325 over 326 keys of 32 heads x 128 in a bf16 cache, span
    [316, 325), D = 4096.  Per round 20 launches of each form between two events, the two forms alternated; us per tail."""
    import ctypes as C
    from anyref_amd import _lib
    lib = _lib.load()
    S, H, hd, e0, s0 = 512, 32, 128, 325, 316
    D = H * hd
    q = torch.randn(1, S, H, hd, device="cuda").bfloat16()
    k = torch.randn(1, S, H, hd, device="cuda").bfloat16()
    hidden = torch.randn(1, S, D, device="cuda")
    y = torch.zeros(1, D, device="cuda")
    items = torch.tensor([[0, e0, s0, 0]], dtype=torch.int32, device="cuda")
    scratch = torch.zeros(1, H, 16, device="cuda")
    kvlen = torch.tensor([e0 + 1], dtype=torch.int32, device="cuda")
    row = torch.zeros(S, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = C.c_int32(0)
    scale = hd ** -0.5

    def chain():
        return lib.anyref_op_rephrase_chain(1, st, P(q), P(k), S, H, hd, P(hidden), 0, e0, s0, P(kvlen), P(row), scale, 0.1, P(y))

    def pair():
        return lib.anyref_op_seg_rephrase(1, st, P(q), P(k), S, H, hd, P(hidden), P(items), 1, e0 - s0, 16, P(scratch), scale, 0.1,
                                          P(y), C.byref(ok))

    us = dict(chain=[], pair=[])
    for r in range(12):
        for name, f in ((("chain", chain), ("pair", pair)) if r % 2 == 0 else (("pair", pair), ("chain", chain))):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                assert f() == 0, lib.anyref_op_last_error().decode()
            b.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / 20)
    assert ok.value == 1
    out = {n: dict(us_median=round(statistics.median(v[2:]), 2), us_min=round(min(v[2:]), 2), us_max=round(max(v[2:]), 2))
           for n, v in us.items()}
    out["shape"] = "e0 325, 32 heads x 128, span 9, bf16 cache; the chain's 4-byte upload is not in its time"
    out["pair_not_above_chain"] = out["pair"]["us_median"] <= out["chain"]["us_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="calls per case and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="perf")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose anyref_amd is measured")
    ap.add_argument("--rephrase", type=float, default=0.0, help="rephrase_weight; > 0: the cases of DESIGN.md §8.9")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from anyref_amd.config import config_7b, IMAGE_TOKEN_INDEX
    from anyref_amd.model import AnyRefForCausalLM
    from anyref_amd.synth import synth_state_dict

    modes = tuple(args.modes.split(","))
    if any(m not in KNOWN for m in modes):
        raise SystemExit("ab_session: --modes takes a comma-separated list of " + ", ".join(KNOWN))
    if not torch.cuda.is_available():
        raise SystemExit("ab_session: needs an MI355X (there is no CPU measurement)")
    dev = torch.device("cuda", 0)
    cfg = config_7b()
    cfg.llm.max_seq = 512
    reph = args.rephrase > 0
    if reph:
        cfg.rephrase_weight = args.rephrase
    sd = synth_state_dict(cfg, seed=0, device=dev, round_bf16=False)
    sd = {k: v.half() if v.is_floating_point() else v for k, v in sd.items()}
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(1, 3, 224, 224, generator=g).to(dev)
    sam = torch.randn(1, 3, 1024, 1024, generator=g).to(dev)
    prefix = torch.cat([torch.tensor([1]), torch.randint(3, 32000, (N_PRE - 2,), generator=g), torch.tensor([IMAGE_TOKEN_INDEX])])
    suffixes = torch.randint(3, 32000, (Q4, N_SUF), generator=g)
    full = torch.cat([prefix, suffixes[0]])[None]
    L = full.shape[1]
    sizes, H, W = [(1024, 1024)], [1024], [1024]
    cases = ("plain",) if args.plain_only else ("plain", "open", "query", "query4", "drafted")
    if reph and not args.plain_only:
        cases = ("plain", "plain_on", "query", "query4", "drafted_plain", "drafted")

    result = {}
    for mode in modes:
        m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=Q4, max_seg=2)
        m.config.eos_token_id = None
        plain = lambda extras=False: m.generate(clip, full, sam, sizes, H, W, max_new_tokens=T_NEW, _return_extras=extras)
        out_ids, _, _ = plain()
        seg_at = 2                                             # bench.py's rule: the id emitted at step 3 is [SEG]
        if reph:                                               # ... or the first later id that is new: a span that is not empty
            a0, old = out_ids[0, L:].tolist(), set(full[0].tolist())
            seg_at = next((i for i in range(2, T_NEW) if a0[i] not in old and a0[i] not in a0[:i]), 2)
        m.set_seg_token_idx(int(out_ids[0, L + seg_at]))
        (out_ids, _, _), ex0 = plain(True)
        answer = out_ids[0, L:].tolist()
        P = len(prefix) + m.n_img - 1
        check, stats = {}, {}
        sess = [None]

        def reopen():
            sess[0] = m.image_session(clip, sam, sizes, H, W, prefix)

        run = dict(plain=lambda: plain(), open=reopen,
                   query=lambda: sess[0].generate(suffixes[:1], max_new_tokens=T_NEW),
                   query4=lambda: sess[0].generate(suffixes, max_new_tokens=T_NEW),
                   drafted=lambda: sess[0].generate(suffixes[:1], max_new_tokens=T_NEW, draft_ids=[answer[:T_NEW - 1]]),
                   plain_on=lambda: plain(),
                   drafted_plain=lambda: m.generate(clip, full, sam, sizes, H, W, max_new_tokens=T_NEW,
                                                    draft_ids=[answer[:T_NEW - 1]]))
        if reph and not args.plain_only:
            m.set_rephrase_paths(True)
        if not args.plain_only:                                # untimed: the session's answer against the plain call's
            reopen()
            for case, rows, draft in (("query", suffixes[:1], None), ("query4", suffixes, None),
                                      ("drafted", suffixes[:1], [answer[:T_NEW - 1]])):
                (o, _, _), ex = sess[0].generate(rows, max_new_tokens=T_NEW, _return_extras=True, draft_ids=draft)
                got = o[0, L:].tolist()
                n = P + N_SUF                                  # the prompt's hidden rows: they depend on no generated id
                scale = ex0["hidden"][0, :n].abs().max().item()
                herr = (ex["hidden"][0, :n] - ex0["hidden"][0, :n]).abs().max().item()
                check[case] = dict(ids_equal_plain=got == answer, prompt_hidden_rows=n, hidden_err=herr, hidden_scale=scale)
                stats[case] = dict(offered=int(ex["draft_offered"][0]), accepted=int(ex["draft_accepted"][0]),
                                   decode_steps=ex["decode_steps"], verify_passes=ex["verify_passes"])
                if mode in PINNED:
                    assert got == answer, f"{mode} / {case}: ids differ from the plain call: {got} vs {answer}"
                assert herr <= HIDDEN_REL * scale, f"{mode} / {case}: hidden err {herr} on a scale of {scale}"

        def prepare(case):                                     # a session query needs an open session; plain ends it
            if reph and not args.plain_only:
                m.set_rephrase_paths(case != "plain")
            if case in ("query", "query4", "drafted"):
                reopen()
                run[case]()                                    # (query4: the broadcast happens once per session, here)

        for case in cases:
            prepare(case)
            for _ in range(args.warmup):
                run[case]()
        torch.cuda.synchronize()
        per = {case: [] for case in cases}
        for r in range(args.rounds):
            for case in (cases if r % 2 == 0 else cases[::-1]):
                prepare(case)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run[case]()
                torch.cuda.synchronize()
                per[case].append((time.perf_counter() - t0) * 1e3 / args.steps / (Q4 if case == "query4" else 1))
        if not args.plain_only:
            sess[0].close()
        med = {case: statistics.median(per[case]) for case in cases}
        result[mode] = {case: dict(
            ms=dict(median=round(med[case], 3), min=round(min(per[case]), 3), max=round(max(per[case]), 3),
                    rounds=[round(x, 3) for x in per[case]]),
            over_plain=round(med[case] / med["plain"], 4), **stats.get(case, {}),
            **({"check": check[case]} if case in check else {})) for case in cases}
        if not args.plain_only:
            result[mode]["query_below_plain_in_every_round"] = all(a < b for a, b in zip(per["query"], per["plain"]))
        if reph:
            result[mode]["seg_at_answer_index"] = seg_at
            result[mode]["first_seg_span"] = answer.index(answer[seg_at])
        del m
        gc.collect()
        torch.cuda.empty_cache()
    bcast = None if args.plain_only else broadcast_alone(torch, cfg, len(prefix) + cfg.clip.n_patches - 1)
    print(json.dumps(dict(
        broadcast_alone=bcast, **(dict(rephrase_weight=args.rephrase, tail_alone=None if args.plain_only else tail_alone(torch))
                                  if reph else {}),
        workload="c2 (7B + ViT-L + SAM-H 1024^2, prefix 291 rows + question 29 = S 320, 10 new tokens), f16-rounded N(0, 0.02^2) "
                 "weights, one handle per mode with max_batch 4; query4 is per query",
        tree=os.path.relpath(os.path.abspath(args.tree), ROOT), plain_only=args.plain_only, rounds=args.rounds, steps=args.steps,
        modes=result)), flush=True)


if __name__ == "__main__":
    main()
