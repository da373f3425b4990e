"""Kernel-level tests of ANYREF_MODE_PARITY16_F16 (include/anyref_hip_ops.h, storage type t = 4): f32 activations carried as a
pair of f16 terms (hi = f16(a), lo = f16(a - hi)) against f16 weights exactly as stored, every reference in float64 on the
SAME f16 weights.

Bounds.  The pair loses |a - hi - lo| <= max(2^-22 |a|, 2^-25) while |a| <= 65504: hi is a's nearest f16 (relative 2^-11 in the
normal range), the residual is exact in f32, and lo is ITS nearest f16 -- relative 2^-11 again, or half an f16 subnormal step
(2^-25) once the residual is below 2^-14.  An f16 weight times an f16 term (11 + 11 bits) is exact in the f32 accumulator, so a
GEMM over the pair is the f32 product to f32 summation error; the project's pair bound PAIR_REL = 3e-5 of the output scale is
kept for it (the bf16 pair's own bound: the f16 pair is finer), and -- as tests/test_gpu_parity16.py does for bf16 -- the result
has to be 20 x inside the same product with A rounded to ONE f16 term.

Mutants: every family also checks that the lo term dropped (a single f16 term) breaks its bound, so these tests cannot stay
green on single-term f16 arithmetic."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_parity16 import P, PAIR_REL, check, close, lib  # noqa: E402,F401

SPH = 4  # storage type id of the f16 pair arithmetic (include/anyref_hip_ops.h)


def h(t):
    return t.to(torch.float16)


def pair_bound(a):
    """what hi + lo may lose of a (float64 tensor in, float64 bound out)"""
    return torch.maximum(a.abs() * 2.0 ** -22, torch.full_like(a, 2.0 ** -25))


def rel_to(ref64, got64):
    return (got64 - ref64).abs().max().item() / max(1.0, ref64.abs().max().item())


GEMM_SHAPES = [
    (4096, 3840, 1280, 0, 1),     # SAM qkv: 256^2 tile
    (4096, 5120, 1280, 2, 0),     # SAM fc1: 256 x 320 tile, GELU, pair-typed output (the next GEMM's A operand)
    (4096, 1280, 5120, 0, 1),     # SAM fc2: 128 x 160 tile
    (320, 12288, 4096, 0, 1),     # prefill qkv: 64 x 256 tile
    (320, 22016, 4096, 0, 1),     # prefill gate / up: whole-M 320 x 96 tile
    (320, 4096, 4096, 0, 1),      # prefill o_proj: split-K slabs
    (320, 4096, 11008, 0, 1),     # prefill down_proj: split-K slabs, K not a power of two
    (257, 4096, 1024, 3, 0),      # CLIP fc1: quick-GELU, pair-typed output
    (257, 1024, 4096, 0, 1),      # CLIP fc2: split-K
    (6, 256, 256, 1, 1), (70, 130, 64, 4, 0), (1000, 64, 192, 0, 0)]


@pytest.mark.parametrize("M,N,K,act,c_f32", GEMM_SHAPES)
def test_f16_pair_gemm_vs_float64(lib, M, N, K, act, c_f32):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + act)
    A = torch.randn(M, K, generator=g) * (1 + torch.rand(M, 1, generator=g) * 4)   # full f32 mantissas, rows of mixed scale
    W = h(torch.randn(N, K, generator=g) * 0.1)
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g) if c_f32 else None
    z = A.double() @ W.double().t() + bias.double()
    acts = [lambda v: v, torch.relu, torch.nn.functional.gelu, lambda v: v * torch.sigmoid(1.702 * v), torch.nn.functional.silu]
    ref = acts[act](z)
    if resid is not None:
        ref = ref + resid.double()
    out = torch.empty(M, N, device="cuda")
    check(lib, lib.anyref_op_gemm(SPH, None, P(A.cuda()), P(W.cuda()), P(bias.cuda()), P(out),
                                  P(resid.cuda()) if resid is not None else None, None, M, N, K, act, c_f32))
    rel = close(out, ref, PAIR_REL, f"gemm {M}x{N}x{K}")
    # mutant: the lo pass dropped = the same product with the activation rounded to ONE f16 term
    z1 = h(A).double() @ W.double().t() + bias.double()
    one = (z1 - z).abs().max().item() / max(1.0, z.abs().max().item())
    mut = acts[act](z1) + (resid.double() if resid is not None else 0.0)
    mrel = rel_to(ref, mut)
    print(f"f16-pair gemm {M}x{N}x{K}: rel err {rel:.2e} (single f16 term: {one:.2e}; mutant through the epilogue {mrel:.2e})")
    assert rel < one / 20
    assert mrel > PAIR_REL, "the mutant (lo pass dropped) stays inside the bound"


def test_f16_pair_gemm_row_map(lib):
    M, N, K = 200, 128, 128
    g = torch.Generator().manual_seed(5)
    A, W = torch.randn(M, K, generator=g), h(torch.randn(N, K, generator=g) * 0.1)
    perm = torch.randperm(M, generator=g).to(torch.int32)
    perm[::7] = -1
    z = A.double() @ W.double().t()
    ref = torch.zeros(M, N, dtype=torch.float64)
    for m in range(M):
        if perm[m] >= 0:
            ref[perm[m]] = z[m]
    out = torch.zeros(M, N, device="cuda")
    check(lib, lib.anyref_op_gemm(SPH, None, P(A.cuda()), P(W.cuda()), None, P(out), None, P(perm.cuda()), M, N, K, 0, 0))
    keep = torch.zeros(M, dtype=torch.bool)
    keep[perm[perm >= 0].long()] = True
    close(out[keep.cuda()], ref[keep], PAIR_REL, "row-mapped pair output")


def test_f16_mfma_subnormal_inputs(lib):
    """Which case is the f16 MFMA in: f16 SUBNORMAL A / B inputs kept or flushed to zero?  (lo = f16(a - hi) is a subnormal
    whenever |a| < ~2^-3, and ~0.3 % of N(0, 1/4096) weights are.)  A: magnitudes in [2^-10, 2^-4) with full f32 mantissas -- hi
    is a normal f16 with ulp <= 2^-15, so EVERY lo term is below 2^-14; W2: every weight a subnormal.  The result is compared
    with the float64 product of the emulated pair (kept) and of the hi terms alone (flushed); both figures are printed, and
    the result has to be one of the two."""
    M, N, K = 320, 512, 4096
    g = torch.Generator().manual_seed(99)
    mag = torch.exp2(torch.rand(M, K, generator=g) * 6 - 10) * (1 + torch.rand(M, K, generator=g)) / 2   # [2^-11, 2^-4)
    A = mag * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1).float()
    hi = h(A)
    lo = h(A - hi.float())
    assert (lo.float().abs() < 2.0 ** -14).all() and (lo != 0).float().mean() > 0.9
    W = h(torch.randn(N, K, generator=g))
    W64 = W.double().t()
    z_pair = (hi.double() + lo.double()) @ W64
    z_hi = hi.double() @ W64
    out = torch.empty(M, N, device="cuda")
    check(lib, lib.anyref_op_gemm(SPH, None, P(A.cuda()), P(W.cuda()), None, P(out), None, None, M, N, K, 0, 1))
    scale = z_pair.abs().max().item()
    d_keep = (out.double().cpu() - z_pair).abs().max().item() / scale
    d_flush = (out.double().cpu() - z_hi).abs().max().item() / scale
    gap = (z_pair - z_hi).abs().max().item() / scale
    case_a = "kept" if d_keep < d_flush else "flushed"
    print(f"f16 MFMA, subnormal A (lo) terms: {case_a} (err vs pair product {d_keep:.2e}, vs hi-only product {d_flush:.2e}, "
          f"the two differ by {gap:.2e} of the output scale)")
    assert min(d_keep, d_flush) < gap / 20, "neither the kept nor the flushed product"
    # subnormal WEIGHTS: |w| < 2^-14 against O(1) activations
    Ws = h((torch.rand(N, K, generator=g) * 2 - 1) * 2.0 ** -15)
    assert (Ws.float().abs() < 2.0 ** -14).all()
    X = torch.randn(M, K, generator=g)
    zs = X.double() @ Ws.double().t()
    out2 = torch.empty(M, N, device="cuda")
    check(lib, lib.anyref_op_gemm(SPH, None, P(X.cuda()), P(Ws.cuda()), None, P(out2), None, None, M, N, K, 0, 1))
    ds = (out2.double().cpu() - zs).abs().max().item() / zs.abs().max().item()
    case_w = "kept" if ds < 0.5 else "flushed"
    print(f"f16 MFMA, subnormal weights: {case_w} (err {ds:.2e} of the product's scale {zs.abs().max().item():.2e}; "
          f"flushed would read 1.0)")
    assert ds < 1e-4 or ds > 0.5, "neither kept nor flushed"


GEMV_SHAPES = [(1, 512, 256, 0, 1), (2, 1000, 688, 1, 1), (1, 12288, 4096, 0, 1), (1, 11008, 4096, 1, 1),
               (1, 4096, 11008, 0, 0), (2, 4096, 4096, 0, 0), (4, 300, 1024, 0, 0), (1, 32007, 4096, 0, 1)]


@pytest.mark.parametrize("B,N,K,dual,norm", GEMV_SHAPES)
def test_f16_pair_gemv_vs_float64(lib, B, N, K, dual, norm):
    """f16 weights exactly as stored x the f32 activation row (never rounded to 16 bits): the decode step of parity16_f16.
    Mutant: the row rounded to one f16 term."""
    g = torch.Generator().manual_seed(B + N + K)
    x = torch.randn(B, K, generator=g)
    W, W2 = h(torch.randn(N, K, generator=g) * 0.05), h(torch.randn(N, K, generator=g) * 0.05)
    gain = 1 + 0.1 * torch.randn(K, generator=g)
    bias = torch.randn(N, generator=g) if not dual and not norm else None
    resid = torch.randn(B, N, generator=g)
    xn32 = x
    if norm:
        xn32 = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * gain   # the kernel's f32 statistics

    def product(xn):
        z = xn @ W.double().t()
        if bias is not None:
            z = z + bias.double()
        if dual:
            z = torch.nn.functional.silu(z) * (xn @ W2.double().t())
        return z + resid.double()

    ref = product(xn32.double())
    y = torch.empty(B, N, device="cuda")
    check(lib, lib.anyref_op_gemv(SPH, None, P(x.cuda()), P(gain.cuda()) if norm else None, 1e-6, P(W.cuda()),
                                  P(W2.cuda()) if dual else None, P(bias.cuda()) if bias is not None else None, P(y),
                                  P(resid.cuda()), B, N, K, 0))
    rel = close(y, ref, 1e-5, f"gemv {B}x{N}x{K}")
    mrel = rel_to(ref, product(h(xn32).double()))
    print(f"f16-pair gemv {B}x{N}x{K} dual={dual} norm={norm}: rel err {rel:.2e}, mutant (x as one f16 term) {mrel:.2e}")
    assert mrel > 1e-5, "the mutant stays inside the bound"


def test_f16_pair_gemv_writes_the_normalised_row(lib):
    """gemv_xn (the lm_head launch): the f32 copy of the RMS-normalised rows, through a row map"""
    B, N, K = 2, 1000, 4096
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, K, generator=g) * 2
    W = h(torch.randn(N, K, generator=g) * 0.05)
    gain = 1 + 0.1 * torch.randn(K, generator=g)
    xn = (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * gain).double()
    y = torch.empty(B, N, device="cuda")
    xn_out = torch.zeros(4, K, device="cuda")
    rm = torch.tensor([3, 1], dtype=torch.int32)
    check(lib, lib.anyref_op_gemv_xn(SPH, None, P(x.cuda()), P(gain.cuda()), 1e-6, P(W.cuda()), None, None, P(y), None, B, N, K,
                                     0, P(xn_out), P(rm.cuda()), K))
    close(y, xn @ W.double().t(), 1e-5, "gemv_xn product")
    close(xn_out[rm.long().cuda()], xn, 2e-6, "normalised rows")
    assert (xn_out[[0, 2]] == 0).all()


def test_f16_pair_convert_unsplit_round_trip(lib):
    """launch_convert<pair> -> launch_unsplit on magnitudes spanning 2^-20 .. 2^15 (both signs, full f32 mantissas, zeros):
    per element within max(2^-22 |a|, 2^-25); the device terms are the round-to-nearest-even f16 of torch, subnormals kept.
    Mutant: the hi term alone."""
    rows, cols = 257, 1000          # (rows padded to whole 64-column blocks)
    g = torch.Generator().manual_seed(17)
    e = torch.randint(-20, 15, (rows, cols), generator=g).float()
    a = torch.exp2(e) * (1 + torch.rand(rows, cols, generator=g)) * (torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1).float()
    a[::13, ::7] = 0.0
    assert a.abs().max().item() < 65504
    out = torch.empty(rows, cols, device="cuda")
    hi_dev = torch.empty(rows, cols, dtype=torch.float16, device="cuda")
    check(lib, lib.anyref_op_split_roundtrip(SPH, None, P(a.cuda()), P(out), P(hi_dev), rows, cols))
    a64, bound = a.double(), pair_bound(a.double())
    err = (out.double().cpu() - a64).abs()
    worst = (err / bound).max().item()
    hi = h(a)
    lo = h(a - hi.float())
    exact = torch.equal(out.cpu(), hi.float() + lo.float())
    mut = ((hi_dev.double().cpu() - a64).abs() / bound).max().item()
    print(f"f16 pair round trip: worst error / bound {worst:.3f}, hi term alone {mut:.3g}; bit-identical to torch's RNE terms "
          f"(subnormals kept): {exact}")
    assert worst <= 1.0
    assert torch.equal(hi_dev.cpu(), hi), "hi is not f16(a)"
    assert mut > 1.0, "the mutant (lo term dropped) stays inside the bound"
    assert exact


@pytest.mark.parametrize("rms", [0, 1])
@pytest.mark.parametrize("M,D", [(5, 64), (300, 192), (257, 1024), (33, 1280), (9, 4096), (7, 688)])
def test_f16_pair_norm_output(lib, rms, M, D):
    """the norm kernels write the f16 pair (rows padded to whole 64-column blocks); read back as hi + lo.  Against float64
    at the bf16 pair test's 2e-5; against the f32 output of the same kernel (t = 0) within the f16 pair's own loss,
    max(2^-22 |y|, 2^-25) -- the bf16 pair's 2^-17 |y| has no absolute floor, which an f16 term below 2^-14 needs.
    Mutant: y as one f16 term."""
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * 3 + 1
    gain, bias = torch.randn(D, generator=g), torch.randn(D, generator=g)
    if rms:
        ref = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * gain
    else:
        ref = torch.nn.functional.layer_norm(x, (D,), gain, bias, 1e-6)
    y = torch.empty(M, D, device="cuda")
    check(lib, lib.anyref_op_norm(SPH, None, P(x.cuda()), P(gain.cuda()), None if rms else P(bias.cuda()), P(y), M, D, 1e-6, rms))
    close(y, ref, 2e-5, "norm")
    y0 = torch.empty(M, D, device="cuda")
    check(lib, lib.anyref_op_norm(0, None, P(x.cuda()), P(gain.cuda()), None if rms else P(bias.cuda()), P(y0), M, D, 1e-6, rms))
    y64, y064 = y.double().cpu(), y0.double().cpu()
    assert ((y64 - y064).abs() <= pair_bound(y064)).all()
    assert not ((h(y0.cpu()).double() - y064).abs() <= pair_bound(y064)).all(), "the mutant stays inside the bound"


@pytest.mark.parametrize("B,H,Sq,Sk,hd,causal", [(2, 4, 257, 257, 64, 0), (1, 4, 320, 320, 128, 1), (2, 4, 196, 196, 80, 0)])
def test_f16_pair_attention_output(lib, B, H, Sq, Sk, hd, causal):
    """f32 attention (products as bf16 pairs, exactly as parity16 runs them) whose output rows are written as f16 pairs (the
    proj / o_proj GEMM's A operand).  Against float64 at the bf16 pair test's 2e-5; the same call with bf16-pair output
    rows (t = 3) differs by no more than the two pairs' losses.  Mutant: o as one f16 term."""
    from test_gpu_ops import ref_attention
    g = torch.Generator().manual_seed(B + H + Sq + hd)
    q, k, v = (torch.randn(B, s, H, hd, generator=g) for s in (Sq, Sk, Sk))
    scale = 1.0 / math.sqrt(hd)
    ref = ref_attention(q.double(), k.double(), v.double(), scale, causal, None, None, None, 0)
    o = torch.empty(B, Sq, H, hd, device="cuda")
    check(lib, lib.anyref_op_attention(SPH, None, P(q.cuda()), P(k.cuda()), P(v.cuda()), P(o), B, H, Sq, Sk, hd, scale, causal,
                                       None, None, None, 0, 0))
    rel = close(o, ref, 2e-5, "attention")
    o3 = torch.empty_like(o)
    check(lib, lib.anyref_op_attention(3, None, P(q.cuda()), P(k.cuda()), P(v.cuda()), P(o3), B, H, Sq, Sk, hd, scale, causal,
                                       None, None, None, 0, 0))
    o64, o364 = o.double().cpu(), o3.double().cpu()
    assert ((o64 - o364).abs() <= pair_bound(o364) + o364.abs() * 2.0 ** -17).all()
    mrel = rel_to(ref.double().cpu(), h(ref.float().cpu()).double())
    print(f"attention with f16-pair output rows hd {hd}: rel err {rel:.2e}, mutant (one f16 term) {mrel:.2e}")
    assert mrel > 2e-5, "the mutant stays inside the bound"


@pytest.mark.parametrize("B,H,size,hd", [(2, 4, 14, 80), (2, 2, 4, 64)])
def test_f16_pair_window_attention_output(lib, B, H, size, hd):
    """SAM windows (rel-pos bias from the f32 tables inside the split-pair kernel) with f16-pair output rows"""
    from test_gpu_ops import ref_attention
    ld = 128
    g = torch.Generator().manual_seed(B * 13 + H + size)
    S = size * size
    q, k, v = (torch.randn(B, S, H, hd, generator=g) for _ in range(3))
    th, tw = torch.randn(2 * size - 1, hd, generator=g) * 0.3, torch.randn(2 * size - 1, hd, generator=g) * 0.3
    idx = torch.arange(size)[:, None] - torch.arange(size)[None, :] + size - 1
    rq = q.double().permute(0, 2, 1, 3).reshape(B, H, size, size, hd)
    rel_h = torch.einsum("bnhwc,hkc->bnhwk", rq, th.double()[idx]).reshape(B, H, S, size)
    rel_w = torch.einsum("bnhwc,wkc->bnhwk", rq, tw.double()[idx]).reshape(B, H, S, size)
    scale = hd ** -0.5
    ref = ref_attention(q.double(), k.double(), v.double(), scale, False, None, rel_h, rel_w, size)
    tab = torch.zeros(2, 2 * size, ld)
    tab[0, : 2 * size - 1, :hd], tab[1, : 2 * size - 1, :hd] = th, tw
    tab = tab.cuda()
    o = torch.empty(B, S, H, hd, device="cuda")
    check(lib, lib.anyref_op_attention_tab(SPH, None, P(q.cuda()), P(k.cuda()), P(v.cuda()), P(o), B, H, S, hd, scale,
                                           P(tab[0]), P(tab[1]), ld, size, size))
    close(o, ref, 2e-5, f"window attention from tables, size {size} hd {hd}")
