"""`perf_int4w` (ANYREF_MODE_PERF_INT4W): the int4 group quantiser is bit-exact against its torch statement
(anyref_amd/quant.py), the int4 decode GEMV is held in float64 against the dequantised weights with a bound derived from the
kernel as written, and the whole generate() agrees with the oracle run on those same dequantised weights."""
import ctypes as C
import dataclasses
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anyref_amd import _lib  # noqa: E402
from anyref_amd.config import LlmConfig, config_tiny  # noqa: E402
from anyref_amd.quant import (INT4_GROUP, dequantize_groups_int4, dequantized_state_dict_int4, is_int4_weight,  # noqa: E402
                              quantize_groups_int4)
from anyref_amd.synth import synth_state_dict  # noqa: E402
from oracle import anyref_oracle as O  # noqa: E402
from test_gpu_e2e import make_inputs, pad, rig_seg  # noqa: E402
from test_gpu_ops import U32, check_bound, d64  # noqa: E402

pytestmark = pytest.mark.gpu
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def ngroups(K):
    return (K + INT4_GROUP - 1) // INT4_GROUP


def device_quant(lib, w):
    """f32 [N, K] on the host -> (nibble rows u8 [N, G * 64], scales bf16 [N, G]) on the device, by the library"""
    N, K = w.shape
    wd = w.cuda()
    q = torch.empty(N, ngroups(K) * 64, dtype=torch.uint8, device="cuda")
    s = torch.empty(N, ngroups(K), dtype=torch.bfloat16, device="cuda")
    assert lib.anyref_op_quant_int4(None, P(wd), N, K, P(q), P(s)) == 0, lib.anyref_op_last_error()
    torch.cuda.synchronize()
    return q, s


@pytest.mark.parametrize("N,K", [(64, 256), (33, 688), (7, 16), (128, 4096)])
def test_quantiser_bit_exact(N, K):
    lib = _lib.load()
    g = torch.Generator().manual_seed(N * K)
    w = torch.randn(N, K, generator=g) * 0.02
    w[0, :] = 0                      # all-zero row -> scale 1, q = 0
    w[1, 0] = 3.0                    # a row dominated by one outlier: the rest of its group rounds to 0
    w[2, :8] = torch.tensor([1e-9, -1e-9, 5e-5, -5e-5, 0.02, -0.02, 1e-3, 7e-4])
    q, s = device_quant(lib, w)
    q_ref, s_ref = quantize_groups_int4(w)
    assert torch.equal(s.cpu().float(), s_ref)
    out = torch.empty(N, K, dtype=torch.bfloat16, device="cuda")
    assert lib.anyref_op_dequant_int4(None, P(q), P(s), N, K, P(out)) == 0, lib.anyref_op_last_error()
    torch.cuda.synchronize()
    want = dequantize_groups_int4(q_ref, s_ref)
    assert torch.equal(want.bfloat16().float(), want)
    # -0 and +0 are the same value: compare bit patterns away from zero, values everywhere
    got = out.cpu()
    assert torch.equal(got.float(), want)
    nz = want != 0
    assert torch.equal(got.view(torch.int16)[nz], want.bfloat16().view(torch.int16)[nz])


@pytest.mark.parametrize("B,N,K,dual,norm", [(1, 512, 256, 0, 1),
                                             (2, 96, 688, 0, 0),        # ragged last group
                                             (1, 688, 256, 1, 1),
                                             (4, 40, 4096, 0, 1),
                                             (3, 33, 11008, 0, 0),      # odd N, fewer rows than the template's NB
                                             (1, 64, 13824, 0, 1),
                                             (2, 130, 5120, 1, 1),
                                             (1, 4096, 4096, 0, 0),     # the wave-pair shape
                                             (6, 100, 256, 0, 0),       # two passes
                                             (2, 2052, 256, 1, 1),      # past the wave-pair rule: one wave per row group
                                             (1, 4100, 256, 0, 1)])
def test_gemv_int4(B, N, K, dual, norm):
    """Reference: float64 of bf16(x_norm) W'^T.  Bound, from gemv_int4_kernel as written (the biased-nibble form):
    a lane takes whole 32-weight blocks.  Per block and batch row it forms  t = -136 xsum + sum_k (136 + q_k) x_k  and adds
    s_g t to its sum.  Every product (136 + q_k) x_k is exact in f32 (8 x 8 significant bits).  Before the cancellation is
    complete a term goes through at most: 6 roundings inside xsum (a 4-value tree per thread + 3 shuffle levels at the stage),
    1 for 136 * xsum, and 32 in the chain of 16 packed dots (counted as one rounding per product, whatever the instruction
    fuses): 39 -> c1 = 40 on terms of size m_k |x_k| with  m_k = s_g (|136 + q_k| + 136).  After it, the value is of the size
    of the true partial sum: 1 rounding for the scale FMA, at most 7 blocks per lane and row (K <= 16384: 512 blocks over 64
    lanes ... the FMA chain), 6 shuffle levels, 1 wave-pair merge: 15 -> c2 = 16 on |x_k| |W'_k|.
        bound = 2^-24 (40 sum_k |x_k| m_k + 16 sum_k |x_k| |W'_k|)        (<= 56 * 2^-24 * sum_k |x_k| m_k)
    plus, with the RMSNorm on, the bf16-boundary `flip` term of test_gpu_ops.test_gemv, and the epilogue as there."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(B + N + K)
    x = torch.randn(B, K, generator=g)
    W, W2 = torch.randn(N, K, generator=g) * 0.05, torch.randn(N, K, generator=g) * 0.05
    gain = 1 + 0.1 * torch.randn(K, generator=g)
    resid = torch.randn(B, N, generator=g)
    (q1, s1), (q2, s2) = quantize_groups_int4(W), quantize_groups_int4(W2)
    n1, sc1 = device_quant(lib, W)
    n2, sc2 = device_quant(lib, W2)
    y = torch.empty(B, N, device="cuda")
    keep = [x.cuda(), gain.cuda(), resid.cuda()]
    rc = lib.anyref_op_gemv_int4(None, P(keep[0]), P(keep[1]) if norm else None, 1e-6, P(n1), P(n2) if dual else None, P(sc1),
                                 P(sc2) if dual else None, P(y), P(keep[2]), B, N, K)
    assert rc == 0, lib.anyref_op_last_error()
    torch.cuda.synchronize()

    xd = d64(x)
    xn64 = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * d64(gain) if norm else xd
    xr = xn64.to(torch.bfloat16).double()
    flip = None
    if norm:
        lo, hi = (xn64 * (1 - 2.0 ** -17)).to(torch.bfloat16).double(), (xn64 * (1 + 2.0 ** -17)).to(torch.bfloat16).double()
        flip = (hi - lo).abs()

    def expand(s):
        return d64(s).repeat_interleave(INT4_GROUP, dim=1)[:, :K]

    def lin(q, s):
        Wd = d64(q.float()) * expand(s)                                   # W' (exact)
        m = expand(s) * ((d64(q.float()) + 136).abs() + 136)
        z = xr @ Wd.t()
        e = U32 * (40 * (xr.abs() @ m.t()) + 16 * (xr.abs() @ Wd.abs().t()))
        if flip is not None:
            e = e + flip @ Wd.abs().t()
        return z, e

    def out_of(qa, sa, qb, sb):
        z1, _ = lin(qa, sa)
        if not dual:
            return z1 + d64(resid)
        z2, _ = lin(qb, sb)
        return torch.nn.functional.silu(z1) * z2 + d64(resid)

    z1, e1 = lin(q1, s1)
    ref64 = out_of(q1, s1, q2, s2)
    if dual:
        z2, e2 = lin(q2, s2)
        sz = torch.nn.functional.silu(z1)
        # |silu'| <= 1.1; the f32 silu (exp, division) and the product within 8 units of 2^-24
        bound = 1.1 * e1 * (z2.abs() + e2) + sz.abs() * e2 + 8 * U32 * (sz * z2).abs() + U32 * ref64.abs()
    else:
        bound = e1 + U32 * ref64.abs()

    def drop32(q):                       # mutant 1: the row's last 32 weights (one 16-byte load) lost
        q = q.clone()
        q[:, -32:] = 0
        return q

    def prev_scale(s):                   # mutant 2: the last group multiplied by the previous group's scale
        s = s.clone()
        s[:, -1] = s[:, -2]
        return s
    tag = f"gemv int4 B={B} N={N} K={K} dual={dual} norm={norm}"
    check_bound(y, ref64, bound, out_of(drop32(q1), s1, drop32(q2), s2), tag + " [last load dropped]")
    check_bound(y, ref64, bound, out_of(q1, prev_scale(s1), q2, prev_scale(s2)), tag + " [last scale from the group before]")


SEED, T_NEW = 65, 3     # chosen on the CPU with the oracle alone: every row's top-2 logit gap >= 0.28 (asserted below)


def _hidden_err(hid, ref_h, n):
    return (hid[:n].cpu() - ref_h).abs().max().item()


def test_generate_int4w_matches_oracle_on_dequantised_weights():
    """config_tiny (llm 256 / 688: down_proj has a ragged last group), weights pre-rounded to bf16.  One oracle run of ten ragged
    prompts on W' = dequantised weights; the handle runs B = 1 and B = 4 (GEMV, one pass), B = 6 (two passes) and B = 10 (MFMA
    decode through the bf16 image).  The arithmetic is `perf`'s on exact weights, so the bound is `perf`'s own error on the same
    inputs and the ORIGINAL weights (against the oracle on those), measured here, times 2."""
    from anyref_amd.model import AnyRefForCausalLM
    cfg = config_tiny()
    assert (cfg.llm.dim, cfg.llm.mlp) == (256, 688) and cfg.llm.layers >= 2
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

    # perf's own error on the original weights: the yardstick
    mp = AnyRefForCausalLM.from_state_dict(cfg, sd_cuda, mode="perf", max_batch=NB, max_seg=4)
    mp.config.eos_token_id = None
    perf_p, perf_d = 0.0, 0.0
    perf_hidden = {}
    for B in (1, 4, 6, 10):
        oi, hid = run(mp, B)
        pe, de, _ = errs(oi, hid, ref0, B)
        perf_p, perf_d = max(perf_p, pe), max(perf_d, de)
        perf_hidden[B] = hid[:, : ref0["hidden"][0].shape[0]].clone()
    perf_bytes = mp.device_bytes
    del mp
    bound = 2 * max(perf_p, perf_d)
    print(f"[perf_int4w] perf on the original weights: prefill hidden err {perf_p:.3e}, decode {perf_d:.3e} -> bound {bound:.3e}")

    # rows whose greedy choice the bound cannot decide: top-2 logit gap of the oracle (on W') <= bound at any step
    lm = sd_dq["lm_head.weight"].float()
    gaps = []
    for b in range(NB):
        top = (ref["hidden"][b][-T_NEW:].float() @ lm.T).topk(2, dim=1).values
        gaps.append((top[:, 0] - top[:, 1]).min().item())
    decided = [g > bound for g in gaps]
    print("[perf_int4w] min top-2 logit gap per row: " + " ".join(f"{g:.3f}" for g in gaps))
    assert sum(not d for d in decided) <= NB // 10, "more than 1 row in 10 has a top-2 gap inside the bound"

    m1 = AnyRefForCausalLM.from_state_dict(cfg, sd_cuda, mode="perf_int4w", max_batch=4, max_seg=4)
    m2 = AnyRefForCausalLM.from_state_dict(cfg, sd_cuda, mode="perf_int4w", max_batch=NB, max_seg=4)
    for m in (m1, m2):
        m.config.eos_token_id = None
    for m, B in ((m1, 1), (m1, 4), (m2, 6), (m2, 10)):
        oi, hid = run(m, B)
        pe, de, same = errs(oi, hid, ref, B)
        print(f"[perf_int4w B={B}] prefill hidden err {pe:.3e}, decode {de:.3e} (bound {bound:.3e}); ids identical: {same}")
        assert pe <= bound and de <= bound, (B, pe, de, bound)
        for b in range(B):
            assert same[b] or not decided[b], f"B={B} row {b}: greedy ids differ from the oracle's (gap {gaps[b]:.3f})"
        # int4 is not bf16: the same call on the original weights differs
        n = ref["hidden"][0].shape[0]
        assert (hid[0, :n] - perf_hidden[B][0, :n]).abs().max().item() > 1e-3
    numel = sum(v.numel() for k, v in sd.items() if is_int4_weight(k))
    assert 0 < m1.inexact_weights < numel, (m1.inexact_weights, numel)
    assert m2.device_bytes < perf_bytes


def test_device_bytes_13b_shaped():
    """two layers at LLaMA-13B's widths: the int4 handle is smaller by at least 1.4 bytes per int4 element (1.5 ideal, minus
    2 / 128 for the scales and ~0.025 for the row pad at K = 5120) less the bf16 image of the largest linear"""
    from anyref_amd.model import AnyRefForCausalLM
    cfg = config_tiny()
    cfg = dataclasses.replace(cfg, llm=LlmConfig(vocab=1000, dim=5120, heads=40, layers=2, mlp=13824, max_seq=512))
    sd = synth_state_dict(cfg, seed=31, scale=0.02)
    sd_cuda = {k: v.cuda() for k, v in sd.items()}
    E = sum(v.numel() for k, v in sd.items() if is_int4_weight(k))
    D = 2 * 2 * 13824 * 5120                                             # gate / up interleaved, bf16
    got = {}
    for mode in ("perf", "perf_int4w"):
        m = AnyRefForCausalLM.from_state_dict(cfg, sd_cuda, mode=mode, max_batch=1, max_seg=4)
        got[mode] = m.device_bytes
        del m
    saved = got["perf"] - got["perf_int4w"]
    print(f"[perf_int4w bytes] perf {got['perf']}, int4w {got['perf_int4w']}: saved {saved} = {saved / E:.4f} B / element (E = {E}, D = {D})")
    assert saved >= 1.4 * E - D, (saved, E, D)


def test_refusals():
    from anyref_amd.model import AnyRefForCausalLM
    lib = _lib.load()
    # mode 6 is a mode: anyref_create succeeds
    cfg = config_tiny()
    sd = synth_state_dict(cfg, seed=3, scale=0.05)
    m = AnyRefForCausalLM.from_state_dict(cfg, {k: v.cuda() for k, v in sd.items()}, mode="perf_int4w", max_batch=1, max_seg=4)
    assert m.mode == _lib.MODE_PERF_INT4W == 6
    assert lib.anyref_mode_name(m.h).decode() == "bf16+int4w, SAM f16"
    del m
    # llm_mlp not a multiple of 16: finalize names the tensor
    cfg = config_tiny()
    cfg = dataclasses.replace(cfg, llm=dataclasses.replace(cfg.llm, mlp=680))
    sd = synth_state_dict(cfg, seed=3, scale=0.05)
    with pytest.raises(RuntimeError, match=r"model\.layers\.0\.mlp\.down_proj\.weight"):
        AnyRefForCausalLM.from_state_dict(cfg, {k: v.cuda() for k, v in sd.items()}, mode="perf_int4w", max_batch=1, max_seg=4)
