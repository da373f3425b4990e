"""Kernel-level tests of the f16 flavours ANYREF_MODE_PERF_F16 runs (include/anyref_hip_ops.h with t = 2): the decode GEMV on
the packed f16 dot, the fused decode attention and its fallback over an f16 KV cache, the prefill RoPE + KV append (plain and
from two split-K slabs), the greedy argmax with an f16 embedding table, and the prefill / CLIP GEMM tile forms.

As in test_gpu_ops.py / test_gpu_decode_ops.py: every reference is float64 over exactly the values the kernel stores (f16 has
11 significant bits; the ulp is clamped at 2^-24 where values are subnormal), every bound sits next to the arithmetic it
follows, and a mutant (one plausible loss) must break each bound."""
import math

import pytest
import torch

from test_gpu_ops import P, check, check_bound, d64, dev, drop_last_k, gemm_acc_bound, rnd, U16, U32
from test_gpu_decode_ops import _argmax_rows, _decode_positions, decode_reference, rope_table, rotate64

pytestmark = pytest.mark.gpu

F16 = 2                          # t of the f16 entries


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def ulp16(x):
    """one unit in the last place of f16 at |x| (float64): 11 significant bits, 2^-24 for subnormals and 0"""
    _, e = torch.frexp(x.abs().clamp_min(1e-30))
    return torch.ldexp(torch.ones_like(x), (e - 11).to(torch.int32)).clamp_min(2.0 ** -24)


def flip16(v):
    """an f32 value within 2^-17 (relative: the f32 norm's own error) of an f16 rounding boundary may round either way;
    the rounding step it may take, per element"""
    lo, hi = (v * (1 - 2.0 ** -17)).to(torch.float16).double(), (v * (1 + 2.0 ** -17)).to(torch.float16).double()
    return (hi - lo).abs()


# ----------------------------------------------------------------------------------------------------------------------
# Decode GEMV (launch_gemv<f16>: v_dot2c_f32_f16)
# ----------------------------------------------------------------------------------------------------------------------
# B, N, K, dual (SwiGLU pair), norm (fused RMSNorm), xn (f32 normalised rows out), resid -- LLaMA-7B's decode shapes:
# qkv 12288 x 4096, gate/up 2 x 11008 x 4096 (22016 interleaved rows), o 4096 x 4096, down 4096 x 11008, lm_head 32000 x 4096;
# 32001 and 4099 are not multiples of the two-row group
GEMV_CASES = [(1, 12288, 4096, 0, 1, 0, 0), (2, 11008, 4096, 1, 1, 0, 0), (3, 4096, 11008, 0, 0, 0, 1),
              (4, 4096, 4096, 0, 0, 0, 1), (1, 32000, 4096, 0, 1, 1, 0), (3, 32001, 4096, 0, 1, 1, 0),
              (4, 22016, 4096, 0, 1, 0, 0), (2, 4099, 11008, 0, 0, 0, 1), (4, 11008, 4096, 1, 1, 0, 0)]


@pytest.mark.parametrize("B,N,K,dual,norm,xn,res", GEMV_CASES)
def test_gemv_f16(lib, B, N, K, dual, norm, xn, res):
    """y = (rmsnorm(x) W^T [silu * (x W2^T)]) + resid with f16 weights and the activation row staged as f16.
    Reference: float64 norm rounded to f16 (plus the either-way rounding step of values at a boundary, flip16).
    Sum over K: every lane runs one f32 chain over K / 64 of the products (dot2: two exact f16 x f16 products per rounding),
    6 shuffle levels and the wave-pair merge: c = K / 32 + 16 roundings of 2^-24 sum_k |x_k w_k|.
    Mutant: the last 8 K columns (one 16-byte load) lost."""
    g = torch.Generator().manual_seed(B * 7 + N + K + dual)
    x = torch.randn(B, K, generator=g)
    W, W2 = torch.randn(N, K, generator=g) * 0.02, torch.randn(N, K, generator=g) * 0.02
    gain = 1 + 0.1 * torch.randn(K, generator=g)
    resid = torch.randn(B, N, generator=g)
    y = torch.empty(B, N, device="cuda")
    R, ld = B + 3, K + 4
    xn0 = torch.randn(R, ld, device="cuda")
    xn_out = xn0.clone()
    rmap = torch.randperm(R, generator=torch.Generator().manual_seed(N))[:B].to(torch.int32).cuda()
    Wd, W2d = dev(W, F16), dev(W2, F16)
    if xn:
        check(lib, lib.anyref_op_gemv_xn(F16, None, P(x.cuda()), P(gain.cuda()), 1e-6, P(Wd), P(W2d) if dual else None,
                                         None, P(y), P(resid.cuda()) if res else None, B, N, K, 0, P(xn_out), P(rmap), ld))
    else:
        check(lib, lib.anyref_op_gemv(F16, None, P(x.cuda()), P(gain.cuda()) if norm else None, 1e-6, P(Wd),
                                      P(W2d) if dual else None, None, P(y), P(resid.cuda()) if res else None, B, N, K, 0))
    xd = d64(x)
    xn64 = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * d64(gain) if norm else xd
    xr = xn64.to(torch.float16).double()
    flip = flip16(xn64) if norm else None
    W64, W264 = d64(rnd(W, F16)), d64(rnd(W2, F16))
    r64 = d64(resid) if res else 0.0

    def lin(Wm):
        z = xr @ Wm.t()
        e = (K / 32 + 16) * U32 * (xr.abs() @ Wm.abs().t())
        if flip is not None:
            e = e + flip @ Wm.abs().t()
        return z, e

    def out_of(W1m, W2m):
        z1, _ = lin(W1m)
        if not dual:
            return z1 + r64
        z2, _ = lin(W2m)
        return torch.nn.functional.silu(z1) * z2 + r64
    z1, e1 = lin(W64)
    ref64 = out_of(W64, W264)
    if dual:
        z2, e2 = lin(W264)
        sz = torch.nn.functional.silu(z1)
        # |silu'| <= 1.1; the f32 silu (exp, division) and the product within 8 units of 2^-24
        bound = 1.1 * e1 * (z2.abs() + e2) + sz.abs() * e2 + 8 * U32 * (sz * z2).abs() + U32 * ref64.abs()
    else:
        bound = e1 + U32 * ref64.abs()
    check_bound(y, ref64, bound, out_of(drop_last_k(W64), drop_last_k(W264)), f"gemv f16 B={B} N={N} K={K} dual={dual}")
    if xn:   # the f32 normalised rows (test_gpu_decode_ops.test_gemv_xn_rows' bound), every other row untouched
        got = xn_out[rmap.long(), :K].double()
        assert (got - xn64).abs().max().item() <= 2e-5 * max(1.0, xn64.abs().max().item())
        other = torch.ones(R, dtype=torch.bool, device="cuda")
        other[rmap.long()] = False
        assert torch.equal(xn_out[other], xn0[other]) and torch.equal(xn_out[rmap.long(), K:], xn0[rmap.long(), K:])


# ----------------------------------------------------------------------------------------------------------------------
# Decode attention over an f16 cache (fused kernel and its fallback)
# ----------------------------------------------------------------------------------------------------------------------
def _kpi16(hd):
    kpi = 512 // (hd // 8)        # 8 f16 per 16-byte load
    return kpi


def decode_bound16(pv, dt, o, pos, hd, fallback):
    """test_gpu_decode_ops.decode_bound for an f16 cache.  Fused: c = ceil(n / KPI) + KPI + 4 roundings of sum P|v| for O and
    for l.  Fallback (generic attention, Sq = 1, f16 MFMA: 16 keys per instruction): one rounding per 4 keys + 64 for the
    merges, and P rounded to f16 before P V: + 2^-11 sum P|v|."""
    n = torch.tensor([p + 1 for p in pos], dtype=torch.float64, device=pv.device)[:, None, None]
    c = (n / 4 + 64) if fallback else (torch.ceil(n / _kpi16(hd)) + _kpi16(hd) + 4)
    bound = 2 * c * U32 * pv + dt + 2 * U32 * o.abs()
    if fallback:
        bound = bound + 2.0 ** -11 * pv
    return bound


def assert_rounded16(got, exact, f32err, what):
    err = (got.double() - exact).abs()
    r = (err / (ulp16(exact) + f32err)).max().item()
    assert r <= 1.0, f"{what}: worst error / (1 ulp + f32 rounding) = {r:.3f}"


@pytest.mark.parametrize("hd,H", [(128, 32), (64, 8)])
@pytest.mark.parametrize("maxS", [512])
def test_decode_attn_f16(lib, hd, H, maxS):
    """decode_attn_kernel<f16> and the fallback (RoPE + append + the generic attention) at ragged positions: row p of
    kc / q_keep within 1 ulp of f16 of the float64 rotation, vc row p = f16(v), every other row bitwise unchanged; the output
    against float64 attention over the stored values.  Mutant: the appended key left out."""
    g = torch.Generator(device="cuda").manual_seed(hd * 5 + H)
    tab_d = rope_table(lib, maxS, hd).cuda()
    scale = hd ** -0.5
    pos_all = _decode_positions(1, hd, maxS)          # the bf16 kernel's batch geometry: same 16-byte loads
    worst = [0.0, 0.0]
    for i0 in range(0, len(pos_all), 12):
        pos = pos_all[i0: i0 + 12]
        pos = pos[::2] + pos[1::2]
        B = len(pos)
        qkv = torch.randn(B, 3 * H * hd, device="cuda", generator=g)
        kc0, vc0, qk0 = ((torch.randn(B, maxS, H, hd, device="cuda", generator=g) * 0.5).half() for _ in range(3))
        pos_d = torch.tensor(pos, dtype=torch.int32, device="cuda")
        for fb in (0, 1):
            kc, vc, qk = kc0.clone(), vc0.clone(), qk0.clone()
            out = torch.full((B, H * hd), float("nan"), device="cuda")
            check(lib, lib.anyref_op_decode_attn(F16, None, P(qkv), B, H, hd, P(pos_d), P(tab_d), P(kc), P(vc), maxS, scale,
                                                 P(out), P(qk), fb))
            bi, pd = torch.arange(B, device="cuda"), pos_d.long()
            for name, new, old in (("kc", kc, kc0), ("vc", vc, vc0), ("q_keep", qk, qk0)):
                keep = torch.ones(B, maxS, dtype=torch.bool, device="cuda")
                keep[bi, pd] = False
                assert torch.equal(new[keep], old[keep]), f"{name}: a row other than the appended one changed"
            x = qkv.view(B, 3, H, hd)
            cs, sn = tab_d[pd, 0][:, None, :], tab_d[pd, 1][:, None, :]
            half = hd // 2
            for name, j, buf in (("q_keep", 0, qk), ("kc", 1, kc)):
                ref, e32 = rotate64(x[:, j, :, :half], x[:, j, :, half:], cs, sn)
                assert_rounded16(buf[bi, pd], ref, e32, f"{name} row p (fallback={fb})")
            assert torch.equal(vc[bi, pd], x[:, 2].half()), "vc row p is not v rounded to f16"
            q = qk[bi, pd].float()
            o, pv, dt = decode_reference(q, kc, vc, pos, H, hd, scale)
            bound = decode_bound16(pv, dt, o, pos, hd, fb)
            assert torch.isfinite(out).all()
            r = ((out.view(B, H, hd).double() - o).abs() / bound).max().item()
            assert r <= 1.0, f"decode attention f16 (fallback={fb}): worst error / bound = {r:.3f}"
            worst[fb] = max(worst[fb], r)
            om, _, _ = decode_reference(q, kc, vc, pos, H, hd, scale, drop=1)
            keep_b = torch.tensor([p > 0 for p in pos], device="cuda")
            assert ((om - o).abs() / bound)[keep_b].max() > 1, "bound too loose to see a dropped appended key"
    print(f"decode_attn f16 hd={hd}: worst error / bound fused {worst[0]:.3g}, fallback {worst[1]:.3g}")


# ----------------------------------------------------------------------------------------------------------------------
# Prefill RoPE + KV append into an f16 cache
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f16_vec", "f16_scalar", "slabs_f16"])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_cache_f16(lib, form, hd):
    """launch_rope_cache<f16> (16-byte kernel, and the scalar one on a misaligned qkv) and launch_rope_cache_slabs<f16>: the two
    f32 slices are summed and rounded to f16 first (what the f16 GEMM's own output would be), then rotated; q_out and the
    appended rows within 1 ulp of f16 of the float64 rotation, v exactly f16(v); nothing else written.  Mutant (slabs): the
    sum rounded to bf16 instead of f16 -- the bf16 mode's rounding -- breaks the bound."""
    B, S, H, maxS = 3, 37, 4, 160
    lens, pos0 = [S, S - 9, 1], [0, 23, maxS - S]
    g = torch.Generator(device="cuda").manual_seed(hd + 3 * len(form))
    tab_d = rope_table(lib, maxS, hd).cuda()
    n = B * S * 3 * H * hd
    slab0 = slab1 = qkv = None
    if form == "slabs_f16":
        slab0 = torch.randn(n, device="cuda", generator=g)
        slab1 = torch.randn(n, device="cuda", generator=g) * 0.25
        xin = (slab0 + slab1).half().float()
        xbf = (slab0 + slab1).bfloat16().float()
    else:
        raw = torch.randn(n + 8, device="cuda", generator=g).half()
        qkv = raw[1: n + 1] if form == "f16_scalar" else raw[:n]
        assert (qkv.data_ptr() % 16 != 0) == (form == "f16_scalar")
        xin = qkv.float()
    x = xin.view(B, S, 3, H, hd)
    q_out0 = torch.randn(B, S, H, hd, device="cuda", generator=g).half()
    kc0, vc0, qk0 = (torch.randn(B, maxS, H, hd, device="cuda", generator=g).half() for _ in range(3))
    q_out, kc, vc, qk = q_out0.clone(), kc0.clone(), vc0.clone(), qk0.clone()
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    pos0_d = torch.tensor(pos0, dtype=torch.int32, device="cuda")
    check(lib, lib.anyref_op_rope_cache(F16, None, P(qkv), P(slab0), P(slab1), B, S, H, hd, P(pos0_d), P(lens_d), P(tab_d),
                                        P(q_out), P(kc), P(vc), maxS, P(qk)))
    half = hd // 2
    written = torch.zeros(B, maxS, dtype=torch.bool, device="cuda")
    qrow = torch.zeros(B, S, dtype=torch.bool, device="cuda")
    mutant = 0.0
    for b in range(B):
        L, p0 = lens[b], pos0[b]
        written[b, p0: p0 + L] = True
        qrow[b, :L] = True
        cs, sn = tab_d[p0: p0 + L, 0][:, None], tab_d[p0: p0 + L, 1][:, None]
        qr, eq = rotate64(x[b, :L, 0, :, :half], x[b, :L, 0, :, half:], cs, sn)
        kr, ek = rotate64(x[b, :L, 1, :, :half], x[b, :L, 1, :, half:], cs, sn)
        assert_rounded16(q_out[b, :L], qr, eq, f"{form} q_out")
        assert_rounded16(qk[b, p0: p0 + L], qr, eq, f"{form} q_keep")
        assert_rounded16(kc[b, p0: p0 + L], kr, ek, f"{form} kc")
        assert torch.equal(vc[b, p0: p0 + L], x[b, :L, 2].half()), f"{form}: v row is not v rounded to f16"
        assert torch.equal(q_out[b, :L], qk[b, p0: p0 + L]), f"{form}: q_keep differs from q_out"
        if slab0 is not None:
            xb = xbf.view(B, S, 3, H, hd)
            kb, _ = rotate64(xb[b, :L, 1, :, :half], xb[b, :L, 1, :, half:], cs, sn)
            mutant = max(mutant, ((kb - kr).abs() / (ulp16(kr) + ek)).max().item())
    if slab0 is not None:
        assert mutant > 1, "bound too loose to see the slab sum rounded to bf16"
    for name, new, old, m in (("q_out", q_out, q_out0, ~qrow), ("kc", kc, kc0, ~written), ("vc", vc, vc0, ~written),
                              ("q_keep", qk, qk0, ~written)):
        assert torch.equal(new[m], old[m]), f"{form}: {name} changed outside the appended rows"


# ----------------------------------------------------------------------------------------------------------------------
# argmax with the next step's embedding row from an f16 table
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(32007, 4096), (1000, 320)])
def test_argmax_next_f16_table(lib, N, D):
    """table dtype 2: x_next = the f16 embedding row of the chosen id widened to f32, bit for bit (read as bf16 it would not
    be), plus the id, pos + 1, row_map and kvlen"""
    M, maxS = 12, 640
    g = torch.Generator().manual_seed(N + D)
    x = _argmax_rows(N, M, g)
    table = (torch.randn(N, D, generator=g) * 0.02).half()
    pos0 = torch.randint(0, maxS - 1, (M,), generator=g, dtype=torch.int32)
    pos = pos0.cuda()
    out = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    x_next = torch.full((M, D), float("nan"), device="cuda")
    row_map = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    kvlen = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    check(lib, lib.anyref_op_argmax(None, P(x.cuda()), M, N, N, P(out), P(pos), P(table.cuda()), 2, D, maxS, P(x_next),
                                    P(row_map), P(kvlen)))
    ids = torch.argmax(x, -1)
    p1 = pos0 + 1
    assert torch.equal(out.cpu(), ids)
    assert torch.equal(pos.cpu(), p1)
    assert torch.equal(row_map.cpu(), torch.arange(M, dtype=torch.int32) * maxS + p1)
    assert torch.equal(kvlen.cpu(), p1 + 1)
    assert torch.equal(x_next.cpu(), table[ids].float())
    assert rc_refused(lib, x, table)


def rc_refused(lib, x, table):
    """a table dtype outside 0 / 1 / 2 is refused"""
    M, N = x.shape
    out = torch.empty(M, dtype=torch.int64, device="cuda")
    pos = torch.zeros(M, dtype=torch.int32, device="cuda")
    xn = torch.empty(M, table.shape[1], device="cuda")
    rm, kv = torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda")
    rc = lib.anyref_op_argmax(None, P(x.cuda()), M, N, N, P(out), P(pos), P(table.cuda()), 3, table.shape[1], 640, P(xn),
                              P(rm), P(kv))
    torch.cuda.synchronize()
    return rc != 0


# ----------------------------------------------------------------------------------------------------------------------
# Prefill / CLIP GEMM tile forms in f16
# ----------------------------------------------------------------------------------------------------------------------
# (M, N, K, c_f32, form the launcher picks): prefill gate/up at one image's prompt (M = 257 / 320, N = 22016: whole-M
# 320 x 96 panels), C3's four-prompt o_proj (1280 x 4096 x 4096: 320 x 64, one tile per CU), qkv at 257 rows (64 x 256),
# CLIP qkv / fc1 (257 x 3072 / 4096 x 1024: 64 x 128)
TILE_CASES = [(257, 22016, 4096, 0, "320x96"), (320, 22016, 4096, 1, "320x96"), (1280, 4096, 4096, 1, "320x64"),
              (257, 12288, 4096, 0, "64x256"), (257, 3072, 1024, 0, "64x128"), (257, 4096, 1024, 1, "64x128")]


@pytest.mark.parametrize("M,N,K,c_f32,form", TILE_CASES)
def test_gemm_f16_tile_forms(lib, M, N, K, c_f32, form):
    """C = A W^T + bias (+ resid) on the f16 LDS-DMA tiles; which form runs is checked on the model's profile table by
    test_gpu_perf_f16.py.  Bound: f32 accumulation (K + 32 roundings of 2^-24 sum |a w|) and, for an f16 output, one more
    rounding of 2^-11.  Mutant: the last 8 K columns lost."""
    g = torch.Generator().manual_seed(M + N + K)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    out = torch.empty(M, N, device="cuda", dtype=torch.float32 if c_f32 else torch.float16)
    check(lib, lib.anyref_op_gemm(F16, None, P(dev(A, F16)), P(dev(W, F16)), P(bias.cuda()), P(out),
                                  P(resid.cuda()) if c_f32 else None, None, M, N, K, 0, c_f32))
    A64, W64 = d64(rnd(A, F16)), d64(rnd(W, F16))
    extra = d64(bias) + (d64(resid) if c_f32 else 0)
    ref64 = A64 @ W64.t() + extra
    acc = gemm_acc_bound(A64, W64, K) + 2 * U32 * ref64.abs()
    bound = acc + (0 if c_f32 else U16[F16] * (ref64.abs() + acc))
    assert math.isfinite(bound.max().item())
    check_bound(out, ref64, bound, A64 @ drop_last_k(W64).t() + extra, f"gemm f16 {form} M={M} N={N} K={K}")
