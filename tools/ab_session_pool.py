#!/usr/bin/env python3
"""A/B of session pools (anyref_session_pool_reserve / _store / _generate_pooled) at C2 (LLaMA-7B + CLIP ViT-L/14
+ SAM-H at 1024^2, 10 new tokens; tools/ab_session.py's weights and prompt shape), on ONE handle per mode (max_batch 4).

The workload is K = 4 images with the same `system + image` prefix shape (36 ids: P = 291 spliced rows) and questions of 29 ids,
served ROUND-ROBIN across the images: the worst case for the single session, which is re-opened at every query.  Per mode the
cases are timed alternately, round after round (`--rounds` x `--steps` queries each, after `--warmup`); every figure is PER QUERY:
  reopen   (a) today's best for this stream: `image_session` re-opened at every image switch, one query each
  plain    (b) plain `generate` per query
  pool1    (c) pool, one query per call: every call is about another image, so every call gathers one row
  pool4    (d) pool, four queries per call, each about a different image (rows stay put: gathers are skipped after the first)
  pool4g   (d') as (d), the assignment rotated by one row per call: every call gathers its four rows
  sess4    (e) the same-image four-query call through `ImageSession.generate` (anyref_session_generate)
  pool4s   (f) (e) through the pool, all rows naming one slot
Before the timing, untimed, every pooled row is checked against the plain call on its image: identical ids in parity16; in the
16-bit modes (ids not pinned) the prompt's hidden rows within the mode's bound (2.5 % of their scale).
Also: the gather launch alone (anyref_op_kv_gather) at the 16-bit cache shape for 1 and 4 rows, with bytes and TB/s, and
`anyref_session_store` alone (events around it, on an open session).

`--unchanged` times only the two paths the pool does not touch -- the plain call and one query on a single open session -- and
needs nothing of the feature: with `--tree DIR` (a checkout of the parent commit, built) it is the parent's side of "they cost what
they cost".

Prints ONE JSON line.

usage: python tools/ab_session_pool.py [--rounds 5] [--steps 8] [--warmup 2] [--modes perf,perf_int4w,parity16] [--unchanged] [--tree DIR]
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
N_PRE, N_SUF, K, Q4 = 36, 29, 4, 4


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), rounds=[round(x, 4) for x in v])


def gather_alone(torch, cfg, P, rows):
    """the gather kernel by itself (anyref_op_kv_gather) at the 16-bit modes' cache shape, max_batch 4: `rows` rows of P positions,
    every layer of K and V, each from another slot of a K-slot pool, between two events.  A WARM repeat: the launches follow one
    another over the same buffers, which for one row approach the size of the memory-side cache; the cold figure is the in-situ
    `gather_ms` of `anyref_session_pool_stats` that the timed cases report"""
    import ctypes as C
    from anyref_amd import _lib
    lib = _lib.load()
    l = cfg.llm
    k = torch.zeros(l.layers, Q4, l.max_seq, l.dim, dtype=torch.bfloat16, device="cuda")
    v = torch.zeros_like(k)
    pool = torch.zeros(K, 2 * l.layers, P, l.dim, dtype=torch.bfloat16, device="cuda")
    table = torch.tensor([[b, P, b, 0] for b in range(rows)], dtype=torch.int32)
    ms = []
    for _ in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = lib.anyref_op_kv_gather(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(k.data_ptr()),
                                     C.c_void_p(v.data_ptr()), l.layers, Q4, l.max_seq, C.c_void_p(pool.data_ptr()), K, P, l.dim, 2,
                                     C.c_void_p(table.data_ptr()), rows, 0)
        e1.record()
        assert rc == 0, lib.anyref_op_last_error().decode()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[2:]
    moved = 2 * (2 * l.layers * P * l.dim * 2) * rows           # read once, written once
    return dict(rows=rows, warm_repeat=True, ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), launches=1,
                bytes_read_and_written=moved, tb_per_s=round(moved / statistics.median(ms) / 1e9, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8, help="queries per case and round (a multiple of 4)")
    ap.add_argument("--warmup", type=int, default=2, help="warm-up passes of 4 queries per case")
    ap.add_argument("--modes", default="perf")
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose anyref_amd is measured")
    args = ap.parse_args()
    if args.steps % Q4:
        raise SystemExit("ab_session_pool: --steps must be a multiple of 4")
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from anyref_amd.config import config_7b, IMAGE_TOKEN_INDEX
    from anyref_amd.model import AnyRefForCausalLM
    from anyref_amd.synth import synth_state_dict

    modes = tuple(args.modes.split(","))
    if any(m not in KNOWN for m in modes):
        raise SystemExit("ab_session_pool: --modes takes a comma-separated list of " + ", ".join(KNOWN))
    if not torch.cuda.is_available():
        raise SystemExit("ab_session_pool: needs an MI355X (there is no CPU measurement)")
    dev = torch.device("cuda", 0)
    cfg = config_7b()
    cfg.llm.max_seq = 512
    sd = synth_state_dict(cfg, seed=0, device=dev, round_bf16=False)
    sd = {k: v.half() if v.is_floating_point() else v for k, v in sd.items()}
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(K, 3, 224, 224, generator=g).to(dev)
    sam = torch.randn(K, 3, 1024, 1024, generator=g).to(dev)
    prefix = torch.cat([torch.tensor([1]), torch.randint(3, 32000, (N_PRE - 2,), generator=g), torch.tensor([IMAGE_TOKEN_INDEX])])
    suffixes = torch.randint(3, 32000, (Q4, N_SUF), generator=g)
    full = lambda q: torch.cat([prefix, suffixes[q]])[None]
    L = N_PRE + N_SUF
    size, H, W = (1024, 1024), 1024, 1024
    cases = ("plain", "query") if args.unchanged else ("reopen", "plain", "pool1", "pool4", "pool4g", "sess4", "pool4s")

    result = {}
    for mode in modes:
        m = AnyRefForCausalLM.from_state_dict(cfg, sd, mode=mode, max_batch=Q4, max_seg=2)
        m.config.eos_token_id = None
        plain = lambda k, q, extras=False: m.generate(clip[k: k + 1], full(q), sam[k: k + 1], [size], [H], [W], max_new_tokens=T_NEW,
                                                      _return_extras=extras)
        out_ids, _, _ = plain(0, 0)
        m.set_seg_token_idx(int(out_ids[0, L + 2]))            # bench.py's rule: the id emitted at step 3 is [SEG]
        P = len(prefix) + m.n_img - 1
        open_live = lambda k: m.image_session(clip[k], sam[k], size, H, W, prefix)
        turn = [0]                                             # the stream's position: image turn % K, question turn // K % 4
        state = dict(sess=None, shift=0)

        def nxt():
            t = turn[0]
            turn[0] += 1
            return t % K, (t // K) % Q4

        def run_reopen():
            k, q = nxt()
            with open_live(k) as s:
                s.generate(suffixes[q: q + 1], max_new_tokens=T_NEW)

        def run_plain():
            k, q = nxt()
            plain(k, q)

        def run_query():
            state["sess"].generate(suffixes[:1], max_new_tokens=T_NEW)

        check, extra = {}, {}
        if not args.unchanged:
            pool = m.session_pool(K, max_prefix_rows=P)
            ps = [pool.open(k, clip[k], sam[k], size, H, W, prefix) for k in range(K)]
            extra["pool"] = {k: v for k, v in pool.stats().items() if k in ("slots", "in_use", "bytes")}
            extra["device_bytes"] = m.device_bytes

            def run_pool1():
                k, q = nxt()
                pool.generate([ps[k]], suffixes[q: q + 1], max_new_tokens=T_NEW)

            def run_pool4():
                pool.generate(ps, suffixes, max_new_tokens=T_NEW)

            def run_pool4g():
                state["shift"] = (state["shift"] + 1) % K
                pool.generate([ps[(b + state["shift"]) % K] for b in range(Q4)], suffixes, max_new_tokens=T_NEW)

            def run_sess4():
                state["sess"].generate(suffixes, max_new_tokens=T_NEW)

            def run_pool4s():
                pool.generate([ps[0]] * Q4, suffixes, max_new_tokens=T_NEW)

            # untimed: a mixed four-row call against the plain calls on each row's image
            (o, _, _), ex = pool.generate(ps, suffixes, max_new_tokens=T_NEW, _return_extras=True)
            rows = []
            for b in range(Q4):
                (po, _, _), pex = plain(b, b, True)
                n = P + N_SUF                                  # the prompt's hidden rows: they depend on no generated id
                scale = pex["hidden"][0, :n].abs().max().item()
                herr = (ex["hidden"][b, :n] - pex["hidden"][0, :n]).abs().max().item()
                same = o[b, L: L + T_NEW].tolist() == po[0, L:].tolist()
                rows.append(dict(ids_equal_plain=same, hidden_err=herr, hidden_scale=scale))
                if mode in PINNED:
                    assert same, f"{mode}: row {b} ids differ from the plain call"
                assert herr <= HIDDEN_REL * scale, f"{mode}: row {b} hidden err {herr} on a scale of {scale}"
            check["pool4"] = rows
            # store alone: the live session of image 0 packed into its slot again, between two events
            st_ms = []
            with open_live(0):
                for _ in range(8):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    m._check(m.lib.anyref_session_store(m.h, m._stream(), ps[0].slot), "session_store")
                    e1.record()
                    torch.cuda.synchronize()
                    st_ms.append(e0.elapsed_time(e1))
            extra["store_alone_ms"] = summary(st_ms[2:])
            ps[0] = pool.open(0, clip[0], sam[0], size, H, W, prefix)      # (the raw stores moved the library's generation on)

        run = dict(reopen=run_reopen, plain=run_plain, query=run_query)
        per_call = dict(reopen=1, plain=1, query=1, pool1=1, pool4=Q4, pool4g=Q4, sess4=Q4, pool4s=Q4)
        if not args.unchanged:
            run.update(pool1=run_pool1, pool4=run_pool4, pool4g=run_pool4g, sess4=run_sess4, pool4s=run_pool4s)

        def prepare(case):
            if state["sess"] is not None:
                state["sess"].close()
                state["sess"] = None
            if case in ("query", "sess4"):                     # a live session; the plain and pooled cases end it
                state["sess"] = open_live(0)
            run[case]()

        gms = {"pool1": [], "pool4g": []}
        for case in cases:
            prepare(case)
            for _ in range(args.warmup * Q4 // per_call[case]):
                run[case]()
        torch.cuda.synchronize()
        per = {case: [] for case in cases}
        for r in range(args.rounds):
            for case in (cases if r % 2 == 0 else cases[::-1]):
                prepare(case)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps // per_call[case]):
                    run[case]()
                torch.cuda.synchronize()
                per[case].append((time.perf_counter() - t0) * 1e3 / args.steps)
                if case in gms:
                    gms[case].append(pool.stats()["gather_ms"])
        if state["sess"] is not None:
            state["sess"].close()
        result[mode] = {case: dict(ms_per_query=summary(per[case])) for case in cases}
        for case, v in gms.items():
            if v and all(x is not None for x in v):
                result[mode][case]["gather_ms_in_situ_last_call"] = summary(v)
        result[mode].update(extra)
        if check:
            result[mode]["check"] = check
        if not args.unchanged:
            result[mode]["pool1_below_reopen_in_every_round"] = all(a < b for a, b in zip(per["pool1"], per["reopen"]))
            e = per["sess4"]
            result[mode]["pool4_minus_sess4_ms"] = round(statistics.median(per["pool4"]) - statistics.median(e), 4)
            result[mode]["pool4g_minus_sess4_ms"] = round(statistics.median(per["pool4g"]) - statistics.median(e), 4)
            result[mode]["pool4s_minus_sess4_ms"] = round(statistics.median(per["pool4s"]) - statistics.median(e), 4)
            result[mode]["sess4_spread_ms"] = round(max(e) - min(e), 4)
            pool.close()
        del m
        gc.collect()
        torch.cuda.empty_cache()
    P = len(prefix) + cfg.clip.n_patches - 1
    print(json.dumps(dict(
        gather_alone=None if args.unchanged else [gather_alone(torch, cfg, P, n) for n in (1, Q4)],
        workload="c2 (7B + ViT-L + SAM-H 1024^2, prefix 291 rows + question 29 = S 320, 10 new tokens), f16-rounded N(0, 0.02^2) "
                 "weights, one handle per mode with max_batch 4, 4 images round-robin; every figure per query",
        tree=os.path.relpath(os.path.abspath(args.tree), ROOT), unchanged_only=args.unchanged, rounds=args.rounds, steps=args.steps,
        modes=result)), flush=True)


if __name__ == "__main__":
    main()
