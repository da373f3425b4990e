"""Proves the bounds of tests/gemm_forms_ref.py without a GPU: for every launch form, at reduced shapes, an f32 emulation
of the kernel (stored operands, an f32 matmul per K slice, slabs summed in slab order, an f32 epilogue, the output rounded
to its storage type) must lie inside the bound, and every mutant must lie outside it -- so no bound is vacuous and none
is tighter than f32 arithmetic allows, before anyone has a card."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_forms_ref as R  # noqa: E402


def both(ty, A, W, losses, key, what, **kw):
    """emulation inside, every mutant outside"""
    out = R.gemm_form(ty, A, W, **kw)
    emu = R.gemm_form(ty, A, W, emulate=True, **kw)
    ref, bound = out[key]
    muts = {name: R.gemm_form(ty, A, W, loss=name, **kw)[key][0] for name in losses}
    return R.check_bound(emu[key], ref, bound, muts, what)


@pytest.mark.parametrize("ty", [1, 2, 3, 4])
@pytest.mark.parametrize("M,N,K,splits,ln", [(24, 256, 2048, 4, False), (9, 192, 1024, 8, False), (17, 128, 1024, 2, True),
                                             (20, 320, 1536, 3, True)])
def test_fused_norm(ty, M, N, K, splits, ln):
    A, W, bias, resid, gain, nbias = R.gemm_operands(M, N, K, M + N + K, small_rows=True, row_offset=ln, with_bias=ln)
    norm = {"gain": gain, "bias": nbias if ln else None, "eps": 1e-6}
    kw = dict(bias=bias if ln else None, resid=resid, c_f32=True, norm=norm, splits=splits)
    losses = ["drop_k", "norm_before_resid", "no_eps"] + (["ln_keeps_mean"] if ln else [])
    both(ty, A, W, losses, "norm", f"cpu fused norm t={ty} {M}x{N}x{K} ln={ln}", **kw)
    both(ty, A, W, ["drop_k"], "C", f"cpu fused norm C t={ty} {M}x{N}x{K}", **kw)
    kw["c_f32"] = False      # a 16-bit / pair-typed C beside the norm
    both(ty, A, W, ["drop_k"], "C", f"cpu fused norm typed C t={ty} {M}x{N}x{K}", **kw)


@pytest.mark.parametrize("ty", [1, 2, 3, 4])
@pytest.mark.parametrize("c_f32", [0, 1])
@pytest.mark.parametrize("M,N,K,splits", [(33, 384, 256, 1), (8, 128, 2048, 4)])
def test_swiglu_pairs(ty, c_f32, M, N, K, splits):
    A, W, *_ = R.gemm_operands(M, N, K, M + N + K + c_f32)
    both(ty, A, W, ["drop_k", "swap_gate_up", "not_interleaved"], "C", f"cpu swiglu t={ty} c_f32={c_f32} {M}x{N}x{K}",
         swiglu=True, c_f32=bool(c_f32), splits=splits)


@pytest.mark.parametrize("ty", [1, 2, 3, 4])
def test_raw_slabs(ty):
    A, W, *_ = R.gemm_operands(40, 192, 512, 11)
    both(ty, A, W, ["drop_k", "slab_swapped", "slab_missing"], "slabs", f"cpu raw slabs t={ty}", slabs=2)


@pytest.mark.parametrize("ty", [1, 2])
def test_batched(ty):
    # rel-pos layout: batch = heads over a shared table
    A, W, bias, resid, *_ = R.gemm_operands(50, 64, 80, 3, Z=4, w_scale=0.3)
    both(ty, A, W, ["drop_k", "z_on_shared_w"], "C", f"cpu batched shared W t={ty}")
    # patch embedding: a residual shared by every batch element
    both(ty, A, W, ["drop_k", "resid_per_batch"], "C", f"cpu batched shared resid t={ty}", bias=bias[:1], resid=resid[:1])
    # per-batch W and bias, ReLU, alpha
    A, W, bias, *_ = R.gemm_operands(20, 96, 128, 4, Z=3, Zw=3)
    both(ty, A, W, ["drop_k", "alpha_ignored"], "C", f"cpu batched bias relu alpha t={ty}", bias=bias, act=R.ACT_RELU,
         alpha=0.125, c_f32=False)


@pytest.mark.parametrize("ty", [1, 2])
def test_capped_row_blocks(ty):
    M, N, K = 768, 64, 64
    A, W, bias, resid, *_ = R.gemm_operands(900, N, K, 5)
    g = torch.Generator().manual_seed(6)
    rows = 1000
    row_map = torch.randperm(rows, generator=g)[:M].to(torch.int32)
    row_map[::9] = -1
    C0 = torch.full((1, rows, N), -777.0)
    both(ty, A[:, :M], W, ["drop_k", "block_shift"], "C", f"cpu capped row_map t={ty}", bias=bias, row_map=row_map, C0=C0,
         c_f32=False, block_rows=256)
    amap = torch.randperm(900, generator=g)[:M].to(torch.int32)
    both(ty, A, W, ["drop_k", "block_shift"], "C", f"cpu capped a_row_map t={ty}", bias=bias, resid=resid[:, :M],
         a_row_map=amap, block_rows=256)


@pytest.mark.parametrize("ty", [1, 2, 3, 4])
@pytest.mark.parametrize("rms,act,D", [(0, R.ACT_GELU, 256), (1, R.ACT_NONE, 1280), (0, R.ACT_NONE, 768)])
def test_norm_forms(ty, rms, act, D):
    M, rows = 37, 50
    g = torch.Generator().manual_seed(D + rms)
    x = torch.randn(M, D, generator=g) * 3 + 1
    x[::5] *= 1e-3 / 3
    gain, bias = 1 + 0.2 * torch.randn(D, generator=g), torch.randn(D, generator=g)
    row_map = torch.randperm(rows, generator=g)[:M].to(torch.int32)
    row_map[::6] = -1
    Y0 = torch.full((rows, D), -777.0)
    kw = dict(rms=bool(rms), act=act, row_map=row_map, Y0=Y0)
    b = None if rms else bias
    ref, bound = R.norm_form(ty, x, gain, b, 1e-6, **kw)
    emu = R.norm_form(ty, x, gain, b, 1e-6, emulate=True, **kw)
    losses = ["row_map_ignored", "no_eps"] + (["act_dropped"] if act else [])
    muts = {n: R.norm_form(ty, x, gain, b, 1e-6, loss=n, **kw)[0] for n in losses}
    R.check_bound(emu, ref, bound, muts, f"cpu norm t={ty} rms={rms} act={act} D={D}")


@pytest.mark.parametrize("ty", [0, 1, 2])
def test_fill_rows(ty):
    g = torch.Generator().manual_seed(1)
    N, ld = 96, 128
    dst0 = torch.full((40, ld), -777.0)
    rows = torch.randperm(40, generator=g)[:11].to(torch.int32)
    bias, gain = torch.randn(N, generator=g), 1 + 0.2 * torch.randn(N, generator=g)
    ref, bound = R.fill_form(ty, dst0, rows, bias, N)
    emu = dst0.clone()
    emu[rows.long(), :N] = R.rnd(bias, ty)
    muts = {n: R.fill_form(ty, dst0, rows, bias, N, gain=gain, loss=n)[0] for n in ("gain_scaled", "rows_unmapped")}
    R.check_bound(emu, ref, bound, muts, f"cpu fill rows t={ty}")


@pytest.mark.parametrize("ty", [1, 2])
def test_raw_slabs_chained_into_rope(ty):
    """slab0 + slab1 -> T -> RoPE: the emulation of the chain inside the bound; a missing slab and a lost K chunk outside"""
    S, H, hd, K = 24, 2, 32, 256
    A, W, *_ = R.gemm_operands(S, 3 * H * hd, K, 21)
    g = torch.Generator().manual_seed(2)
    ang = torch.rand(S, hd // 2, generator=g) * 6
    cs, sn = ang.cos(), ang.sin()
    emu_sl = R.gemm_form(ty, A, W, slabs=2, emulate=True)["slabs"]
    emu = R.rope_chain_emulate(ty, emu_sl[0].view(S, 3, H, hd), emu_sl[1].view(S, 3, H, hd), cs, sn)

    def chain(loss=None):
        ref, bnd = R.gemm_form(ty, A, W, slabs=2, loss=loss)["slabs"]
        return R.rope_chain_form(ty, ref.sum(0).view(S, 3, H, hd), bnd.sum(0).view(S, 3, H, hd), cs, sn)
    out, m1, m2 = chain(), chain("slab_missing"), chain("drop_k")
    for key in ("q", "k", "v"):
        R.check_bound(emu[key], out[key][0], out[key][1], {"slab_missing": m1[key][0], "drop_k": m2[key][0]},
                      f"cpu slabs -> rope t={ty} {key}")


@pytest.mark.parametrize("ty", [1, 2, 3])
def test_attention_forms(ty):
    B, H, S, hd = 3, 2, 70, 16
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(B, S, H, hd, generator=g) for _ in range(3))
    if ty != 3:      # (t = 3 takes full f32 operands)
        q, k, v = (R.rnd(x, ty) for x in (q, k, v))
    scale = hd ** -0.5
    # fused-qkv strides: a kernel that reads k at the q offset attends over q
    ref, bound = R.attention_form(ty, q, k, v, scale, tile=16)
    emu = R.attention_emulate(ty, q, k, v, scale, tile=16)
    muts = {n: R.attention_form(ty, q, k, v, scale, loss=n, k_wrong=q, tile=16)[0] for n in ("drop_tile", "k_wrong")}
    R.check_bound(emu, ref, bound, muts, f"cpu attention fused strides t={ty}")
    # ragged prefill: causal, rows >= q_len keep their sentinel exactly
    lens, p0 = torch.tensor([70, 33, 1], dtype=torch.int32), torch.tensor([0, 20, 5], dtype=torch.int32)
    O0 = torch.full((B, S, H, hd), -768.0)
    kw = dict(causal=True, kv_len=lens + p0, q_len=lens, q_pos0=p0, O0=O0, tile=16)
    ref, bound = R.attention_form(ty, q, k, v, scale, **kw)
    emu = R.attention_emulate(ty, q, k, v, scale, **kw)
    muts = {n: R.attention_form(ty, q, k, v, scale, loss=n, **kw)[0] for n in ("drop_tile", "q_len_ignored", "q_pos0_ignored")}
    R.check_bound(emu, ref, bound, muts, f"cpu attention ragged prefill t={ty}")
