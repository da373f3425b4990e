"""The int4-operand MFMA GEMM (the W4 form of gemm_glds_kernel) and `perf_int4w` on top of it.

Op level (`anyref_op_gemm_int4`): held in float64 against the dequantised weights, and bit for bit against the bf16 GEMM on
the bf16 image of the same nibbles.  End to end: config_tiny with llm_mlp = 704 (every int4 linear has K % 64 == 0, so no
linear takes the image fallback) against the oracle on the dequantised weights; and the handle's size at 13B widths."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anyref_amd import _lib  # noqa: E402
from anyref_amd.config import LlmConfig, config_tiny  # noqa: E402
from anyref_amd.quant import (dequantize_groups_int4, dequantized_state_dict_int4, is_int4_weight, pack_groups_int4,  # noqa: E402
                              quantize_groups_int4)
from anyref_amd.synth import synth_state_dict  # noqa: E402
from oracle import anyref_oracle as O  # noqa: E402
from test_gpu_e2e import make_inputs, pad, rig_seg  # noqa: E402
from test_gpu_int4w import device_quant  # noqa: E402
from test_gpu_ops import U16, U32, check_bound, d64, gemm_acc_bound  # noqa: E402

pytestmark = pytest.mark.gpu
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

# (M, N, K, form, tile): form "f32" plain f32 output, "bias" f32 + bias, "resid" f32 + residual, "swiglu" interleaved gate / up
# rows -> bf16 [M, N / 2].  `tile` is the launch tag the shape must book (anyref_op_last_tags): which instantiation it reaches.
SHAPES = [
    (64, 128, 64, "f32", "gemm_bf16_128x128s3_int4w"),          # one K tile, half a group
    (65, 200, 192, "bias", "gemm_bf16_128x128s3_int4w"),        # ragged M / N; 1.5 groups: the scale changes between tiles 1 and 2
    (33, 136, 192, "swiglu", "gemm_bf16_128x128s3_int4w"),      # SwiGLU pairs, bf16 output
    (10, 256, 256, "f32", "gemm_bf16_128x128s3_int4w_dec"),     # decode rows
    (16, 4160, 320, "f32", "gemm_bf16_128x128s3_int4w_dec"),
    (64, 128, 2176, "resid", "gemm_bf16_128x128s3_int4w"),      # split-K by 2: slices of 1088 = 8.5 groups, slice 1 starts mid-group
    (320, 4096, 2752, "f32", "gemm_bf16_128x128s3_int4w"),      # the down_proj slice width (21.5 groups)
    # one shape per further tile instantiation the launcher reaches with an int4 operand
    (16, 8192, 128, "f32", "gemm_bf16_64x256s3_int4w_dec"),     # 64 x 256, three stages (decode gate / up, prefill qkv)
    (320, 13312, 64, "f32", "gemm_bf16_64x256_int4w"),          # 64 x 256, two stages (more tiles than CUs)
    (576, 6656, 64, "f32", "gemm_bf16_128x128g_int4w"),         # 128 x 128, two stages
    (1024, 13312, 64, "f32", "gemm_bf16_256x256_int4w"),        # 256 x 256 (prefill at M = B S)
    (200, 16384, 128, "f32", "gemm_bf16_320x96s3_int4w"),       # whole-M gate / up tile
    (200, 4096, 2048, "f32", "gemm_bf16_320x64_int4w"),         # whole-M split-K slabs (4 slices of 512: only reachable at K >= 2048)
    (200, 4096, 2304, "f32", "gemm_bf16_320x64_int4w"),         # the same tile, 4 slices of 576 = 4.5 groups: slices 1 and 3 start mid-group
]
IDS = [f"{m}x{n}x{k}-{f}" for m, n, k, f, _ in SHAPES]


@functools.lru_cache(maxsize=None)
def case(M, N, K, form):
    """inputs on the host, the quantised weight on the device (by the library's quantiser), and ONE run of the op"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn(M, K, generator=g).bfloat16()
    W = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g) if form == "bias" else None
    resid = torch.randn(M, N, generator=g) if form == "resid" else None
    q, s = quantize_groups_int4(W)
    nib, sc = device_quant(lib, W)
    assert torch.equal(nib.cpu(), pack_groups_int4(q)) and torch.equal(sc.cpu().float(), s)
    swiglu = form == "swiglu"
    out = torch.empty(M, N // 2, dtype=torch.bfloat16, device="cuda") if swiglu else torch.empty(M, N, device="cuda")
    dev = dict(A=A.cuda(), bias=bias.cuda() if bias is not None else None, resid=resid.cuda() if resid is not None else None)
    rc = lib.anyref_op_gemm_int4(None, P(dev["A"]), P(nib), P(sc), P(dev["bias"]), P(out), P(dev["resid"]), M, N, K, 0,
                                 0 if swiglu else 1, 1 if swiglu else 0)
    assert rc == 0, lib.anyref_op_last_error()
    torch.cuda.synchronize()
    tags = lib.anyref_op_last_tags().decode()
    return dict(A=A, q=q, s=s, bias=bias, resid=resid, nib=nib, sc=sc, out=out, tags=tags, dev=dev)


@pytest.mark.parametrize("M,N,K,form,tile", SHAPES, ids=IDS)
def test_gemm_int4_vs_float64(M, N, K, form, tile):
    """Reference: float64 of bf16(A) W'^T, W' = q * s.  The operand fragments are exactly W' and every bf16 x bf16 product is
    exact in f32, as for a bf16 weight, so the bound is gemm_acc_bound(A, W', K) = (K + 32) 2^-24 sum_k |a_k w'_k| -- its + 32
    covers the split-K sum, the bias add (K = 192: |bias| <= 5 against sum_k |a_k w'_k| ~ 6) and the residual add (K = 2176:
    |resid| <= 5 against ~ 70), one f32 rounding each.  A bf16 output adds half an ulp of the (computed) value; the SwiGLU form propagates the two accumulation errors
    through silu (|silu'| <= 1.1; the f32 silu and product within 8 units of 2^-24), as test_gemv_int4 does.
    Mutants that must break the bound: the row's last 64-k tile dropped; the last group multiplied by the previous group's
    scale (left out at K = 64: one group); for SwiGLU also gate and up swapped.
    Tiles reached (asserted on the launch tag): the seven issue shapes run on 128 x 128 s3 (K = 2176 as two split-K slices);
    16 x 8192 -> 64 x 256 s3, 320 x 13312 -> 64 x 256, 576 x 6656 -> 128 x 128 g, 1024 x 13312 -> 256 x 256,
    200 x 16384 -> 320 x 96 s3, 200 x 4096 x 2048 and x 2304 -> 320 x 64 on four split-K slices (2304: down_proj's case of
    slices that start mid-group, on the tile down_proj takes)."""
    c = case(M, N, K, form)
    assert tile in c["tags"].split(","), c["tags"]
    A64 = d64(c["A"].float())
    G = c["s"].shape[1]

    def wd(q, s):
        return d64(dequantize_groups_int4(q, s))

    def z_of(Wd):
        z = A64 @ Wd.t()
        if c["bias"] is not None:
            z = z + d64(c["bias"])
        if c["resid"] is not None:
            z = z + d64(c["resid"])
        return z

    def out_of(Wd, swap=False):
        z = z_of(Wd)
        if form != "swiglu":
            return z
        gate, up = (z[:, 1::2], z[:, 0::2]) if swap else (z[:, 0::2], z[:, 1::2])
        return torch.nn.functional.silu(gate) * up

    Wd = wd(c["q"], c["s"])
    ref64 = out_of(Wd)
    e = gemm_acc_bound(A64, Wd, K)
    if form == "swiglu":
        z = z_of(Wd)
        z1, z2, e1, e2 = z[:, 0::2], z[:, 1::2], e[:, 0::2], e[:, 1::2]
        sz = torch.nn.functional.silu(z1)
        acc = 1.1 * e1 * (z2.abs() + e2) + sz.abs() * e2 + 8 * U32 * (sz * z2).abs() + U32 * ref64.abs()
        bound = acc + U16[1] * (ref64.abs() + acc)
    else:
        bound = e
    q_drop = c["q"].clone()
    q_drop[:, -64:] = 0
    tag = f"gemm int4 {M}x{N}x{K} {form}"
    check_bound(c["out"], ref64, bound, out_of(wd(q_drop, c["s"])), tag + " [last 64-k tile dropped]")
    if G >= 2:
        s_prev = c["s"].clone()
        s_prev[:, -1] = s_prev[:, -2]
        check_bound(c["out"], ref64, bound, out_of(wd(c["q"], s_prev)), tag + " [last scale from the group before]")
    if form == "swiglu":
        check_bound(c["out"], ref64, bound, out_of(Wd, swap=True), tag + " [gate and up swapped]")


@pytest.mark.parametrize("M,N,K,form,tile", [s for s in SHAPES if s[3] != "swiglu"], ids=[i for i in IDS if "swiglu" not in i])
def test_gemm_int4_bitwise_equals_bf16_image(M, N, K, form, tile):
    """anyref_op_dequant_int4 + the bf16 GEMM on the image == the int4-operand GEMM on the nibbles, f32 bit for bit: same
    operand values, same MFMA, same k order, same split-K rule (no shape here needs two different K splits)"""
    lib = _lib.load()
    c = case(M, N, K, form)
    img = torch.empty(N, K, dtype=torch.bfloat16, device="cuda")
    assert lib.anyref_op_dequant_int4(None, P(c["nib"]), P(c["sc"]), N, K, P(img)) == 0, lib.anyref_op_last_error()
    out = torch.empty(M, N, device="cuda")
    rc = lib.anyref_op_gemm(1, None, P(c["dev"]["A"]), P(img), P(c["dev"]["bias"]), P(out), P(c["dev"]["resid"]), None, M, N, K, 0, 1)
    assert rc == 0, lib.anyref_op_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), c["out"].view(torch.int32)), \
        f"{(out - c['out']).abs().max().item():.3e} apart on {(out != c['out']).sum().item()} elements"


def test_gemm_int4_refuses_what_the_form_cannot_take():
    lib = _lib.load()
    M, N, K = 8, 64, 96                                   # K % 64 != 0: an error, never a fallback
    A = torch.zeros(M, K, dtype=torch.bfloat16, device="cuda")
    nib = torch.full((N, 64), 0x88, dtype=torch.uint8, device="cuda")
    sc = torch.ones(N, 1, dtype=torch.bfloat16, device="cuda")
    out = torch.empty(M, N, device="cuda")
    assert lib.anyref_op_gemm_int4(None, P(A), P(nib), P(sc), None, P(out), None, M, N, K, 0, 1, 0) != 0
    assert b"int4" in lib.anyref_op_last_error()
    M, N, K = 8, 65, 64                                   # N * ceil(K / 128) odd: the last scale's aligned dword would end past the array
    A = torch.zeros(M, K, dtype=torch.bfloat16, device="cuda")
    nib = torch.full((N, 64), 0x88, dtype=torch.uint8, device="cuda")
    sc = torch.ones(N + 1, 1, dtype=torch.bfloat16, device="cuda")
    out = torch.empty(M, N, device="cuda")
    assert lib.anyref_op_gemm_int4(None, P(A), P(nib), P(sc), None, P(out), None, M, N, K, 0, 1, 0) != 0
    assert b"must be even" in lib.anyref_op_last_error()


SEED, T_NEW = 94, 3     # chosen on the CPU with the oracle alone: top-2 logit gaps 0.152, 0.193 and >= 0.245 on the other 8 rows


def test_generate_int4w_all_linears_through_the_int4_gemm():
    """config_tiny with llm_mlp = 704 (5.5 groups; every int4 linear has K % 64 == 0), the method of
    test_generate_int4w_matches_oracle_on_dequantised_weights: oracle on W' = dequantised weights, bound = 2 x `perf`'s own
    hidden-state error on the original weights, measured here.  B = 1 (int4 GEMM prefill, GEMV decode) and B = 10 (int4 GEMM
    prefill at M = B S, int4 GEMM decode rows inside the graph); one ragged llm_forward; and the B = 1 call books int4 GEMM
    launches in the profile."""
    from anyref_amd.model import AnyRefForCausalLM
    cfg = config_tiny()
    cfg = dataclasses.replace(cfg, llm=dataclasses.replace(cfg.llm, mlp=704))
    assert (cfg.llm.dim, cfg.llm.mlp) == (256, 704) and cfg.llm.layers >= 2
    sd = synth_state_dict(cfg, seed=SEED, scale=0.05)
    sd = {k: (v.bfloat16().float() if v.is_floating_point() else v) for k, v in sd.items()}
    sd["lm_head.weight"] = sd["lm_head.weight"] * 4
    sd_dq = dequantized_state_dict_int4(sd)
    NB = 10
    clip, sam, ids = make_inputs(cfg, NB, seed=SEED + 1, L=32)
    sizes, H, W = [(224, 224)] * NB, [224] * NB, [224] * NB
    rig_seg(cfg, sd_dq, clip, sam, ids, sizes, (H, W))
    with torch.no_grad():
        ref = O.anyref_generate(sd_dq, cfg, clip, ids, sam, sizes, H, W, max_new_tokens=T_NEW, eos=False)
        ref0 = O.anyref_generate(sd, cfg, clip, ids, sam, sizes, H, W, max_new_tokens=T_NEW, eos=False)
    padded, mask = pad(ids)
    sd_cuda = {k: v.cuda() for k, v in sd.items()}

    def run(m, B):
        (oi, _, _), ex = m.generate(clip[:B], padded[:B], sam[:B], sizes[:B], H[:B], W[:B], max_new_tokens=T_NEW,
                                    attention_masks=mask[:B], _return_extras=True)
        return oi, ex["hidden"]

    def errs(oi, hid, r, B):
        """worst prefill / decode hidden error over rows 0 .. B - 1 (decode rows only while the ids agree), ids per row"""
        pe, de, same = 0.0, 0.0, []
        for b in range(B):
            want, wid = r["hidden"][b], r["output_ids"][b].tolist()
            Sp = len(ids[b]) + cfg.clip.n_patches - 1
            got = hid[b, : want.shape[0]].cpu()
            pe = max(pe, (got[:Sp] - want[:Sp]).abs().max().item())
            ok = oi[b, : len(wid)].cpu().tolist() == wid
            same.append(ok)
            if ok:
                de = max(de, (got[Sp:] - want[Sp:]).abs().max().item())
        return pe, de, same

    mp = AnyRefForCausalLM.from_state_dict(cfg, sd_cuda, mode="perf", max_batch=NB, max_seg=4)
    mp.config.eos_token_id = None
    perf_p, perf_d = 0.0, 0.0
    for B in (1, NB):
        oi, hid = run(mp, B)
        pe, de, _ = errs(oi, hid, ref0, B)
        perf_p, perf_d = max(perf_p, pe), max(perf_d, de)
    del mp
    bound = 2 * max(perf_p, perf_d)
    print(f"[int4 gemm e2e] perf on the original weights: prefill hidden err {perf_p:.3e}, decode {perf_d:.3e} -> bound {bound:.3e}")

    lm = sd_dq["lm_head.weight"].float()
    gaps = []
    for b in range(NB):
        top = (ref["hidden"][b][-T_NEW:].float() @ lm.T).topk(2, dim=1).values
        gaps.append((top[:, 0] - top[:, 1]).min().item())
    decided = [g > bound for g in gaps]
    print("[int4 gemm e2e] min top-2 logit gap per row: " + " ".join(f"{g:.3f}" for g in gaps))
    assert sum(not d for d in decided) <= NB // 10, "more than 1 row in 10 has a top-2 gap inside the bound"

    m = AnyRefForCausalLM.from_state_dict(cfg, sd_cuda, mode="perf_int4w", max_batch=NB, max_seg=4)
    m.config.eos_token_id = None
    for B in (1, NB):
        if B == 1:
            m.profile_enable(True)
        oi, hid = run(m, B)
        if B == 1:
            tags = sorted(m.profile_read())
            m.profile_enable(False)
            print("[int4 gemm e2e] B = 1 tags: " + " ".join(tags))
            assert any(t.startswith("gemm_") and "_int4w" in t for t in tags), tags
        pe, de, same = errs(oi, hid, ref, B)
        print(f"[int4 gemm e2e B={B}] prefill hidden err {pe:.3e}, decode {de:.3e} (bound {bound:.3e}); ids identical: {same}")
        assert pe <= bound and de <= bound, (B, pe, de, bound)
        for b in range(B):
            assert same[b] or not decided[b], f"B={B} row {b}: greedy ids differ from the oracle's (gap {gaps[b]:.3f})"

    # llm_forward, B = 2, ragged: against the oracle's hidden states on W'
    g = torch.Generator().manual_seed(SEED + 2)
    S, lens = 40, [40, 27]
    emb = torch.randn(2, S, cfg.llm.dim, generator=g) * 0.05
    r = m.llm_forward(emb, lens=lens)
    for b, n in enumerate(lens):
        with torch.no_grad():
            want, _ = O.llama_layers(sd_dq, cfg, emb[b, :n])
        err = (r["hidden"][b, :n].cpu() - want).abs().max().item()
        print(f"[int4 gemm e2e llm_forward row {b}] hidden err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (b, err, bound)


def test_device_bytes_13b_shaped_without_an_image_buffer():
    """two layers at LLaMA-13B's widths (5120 / 13824: every K % 64 == 0): the int4 handle is smaller than `perf`'s by at least
    1.4 bytes per int4 element (1.5 ideal, minus 2 / 128 for the scales and ~0.025 for the row pad at K = 5120) -- no bf16
    image of any linear is held"""
    from anyref_amd.model import AnyRefForCausalLM
    cfg = config_tiny()
    cfg = dataclasses.replace(cfg, llm=LlmConfig(vocab=1000, dim=5120, heads=40, layers=2, mlp=13824, max_seq=512))
    sd = synth_state_dict(cfg, seed=31, scale=0.02)
    sd_cuda = {k: v.cuda() for k, v in sd.items()}
    E = sum(v.numel() for k, v in sd.items() if is_int4_weight(k))
    got = {}
    for mode in ("perf", "perf_int4w"):
        m = AnyRefForCausalLM.from_state_dict(cfg, sd_cuda, mode=mode, max_batch=1, max_seg=4)
        got[mode] = m.device_bytes
        del m
    saved = got["perf"] - got["perf_int4w"]
    print(f"[int4 gemm bytes] perf {got['perf']}, int4w {got['perf_int4w']}: saved {saved} = {saved / E:.4f} B / element (E = {E})")
    assert saved >= 1.4 * E, (saved, E)
