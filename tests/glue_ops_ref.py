"""Float64 references, derived per-element bounds and mutants for the skinny f32 GEMV and the glue kernels that only the
model's own call paths reach: the mask-decoder tails, the LLM input assembly and the tower front ends
(tests/test_gpu_glue_ops.py runs the kernels against them through the anyref_op_* entry points, tests/test_cpu_glue_ops_ref.py
proves on the CPU that every bound admits an f32 emulation of the kernel and rejects every mutant).  Plain torch; nothing here
needs a GPU or the HIP library.

The conventions are those of tests/gemm_forms_ref.py: the reference is float64 over the operands AS STORED, a bound is a sum
of terms each written down where it is added, none is tuned to what a kernel returns, and a mutant is the reference with
one plausible loss (`loss=`).  `emulate=True` does the arithmetic in f32 in the kernel's own order.

Two kinds of kernel:
  exact    data movement, a widening, one rounding to the storage type or ONE IEEE f32 add: the bound is zero and results are
           compared bit for bit (check_exact).  Their emulation walks the kernel's flat index, so the reference (written with
           tensor indexing) is checked against the kernel's index arithmetic before any card is involved.
  bounded  gemv_skinny, upscale1, upscale2_masks, dense_pe, l2norm_scale: (reference, bound) for check_bound.
"""
import math

import torch

import gemm_forms_ref as G
from gemm_forms_ref import U32, ratio, check_bound, norm_form, out_round_bound, terms  # noqa: F401  (re-exported)

ACT_NONE, ACT_RELU, ACT_GELU, ACT_QUICK_GELU, ACT_SILU = 0, 1, 2, 3, 4
NAN_BITS = 0x7FC12345            # the guard pattern of the GPU tests: a quiet NaN no kernel produces


def nan_fill(shape, dtype=torch.float32, device="cpu"):
    """a buffer of `dtype` whose every 32-bit word (16-bit types: both halves) is a fixed NaN pattern"""
    if dtype == torch.float32:
        return torch.full(shape, NAN_BITS, dtype=torch.int32, device=device).view(torch.float32)
    return torch.full(shape, 0x7FC1, dtype=torch.int16, device=device).view(dtype)


def bits(t):
    """the tensor's words as integers (f32 -> i32, 16-bit -> i16, integers as they are)"""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.contiguous().view(torch.int16)
    return t


def check_exact(got, ref, mutants, what):
    """bit-for-bit equality of `got` with `ref` (same dtype), no element excluded; every mutant must differ from the
    reference somewhere, which proves that the inputs tell the cases apart"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    ref = ref.to(got.device)
    bad = (bits(got) != bits(ref))
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} of {bad.numel()} words differ, first at {bad.nonzero()[0].tolist()}"
    for name, m in (mutants or {}).items():
        m = m.to(got.device).to(ref.dtype)
        assert m.shape == ref.shape, (what, name)
        assert (bits(m) != bits(ref)).any(), f"{what}: the mutant '{name}' equals the reference -- the inputs cannot see it"
    print(f"{what}: exact; mutants " + (", ".join(f"{k} differs" for k in mutants) if mutants else "none"))
    return 0.0


def store(v, ty):
    """an f32 value as the storage type t = 0 .. 4 keeps it, as f32: itself, its RNE to bf16 / f16, or hi + lo of the pair"""
    return G.round_out(v.float(), ty)


def sdtype(ty):
    """dtype of an output buffer at the entry point (pairs come back as f32 = hi + lo)"""
    return torch.float32 if ty in (0, 3, 4) else G.wdtype(ty)


def _fma(acc, a, b):
    """f32 fmaf(a, b, acc): the f32 x f32 product is exact in float64, one rounding of the sum (double rounding aside)"""
    return (acc.double() + a.double() * b.double()).float()


def _butterfly(v):
    """wave_sum over the last axis (64 lanes): v += shfl_xor(v, o) for o = 32 .. 1, every lane ends with the total"""
    o = 32
    idx = torch.arange(64)
    while o:
        v = v + v[..., idx ^ o]
        o >>= 1
    return v


# =====================================================================================================================
# gemv_skinny: launch_gemv_skinny_f32 = gemv_kernel<float, NB, false, 8, false, PAIR = true>
# =====================================================================================================================
GEMV_CH = 1024       # K elements a wave sweeps per chunk: 64 lanes x 4 floats x UNR = 4


def gemv_skinny(xbuf, ldx, W, bias, resid, act, B, *, loss=None, emulate=False):
    """xbuf: the flat f32 buffer x lives in (row b at b * ldx), W [N, K], bias [N] or None, resid [B, N] or None.
    z = x W^T + bias, ref = act(z) + resid.
    bound: per lane one FMA chain over <= K / 64 products (16-byte loads of 4 floats strided over 64 lanes, the wave pair
    halves it again), 6 butterfly levels, the pair merge, the bias add: (K / 64 + 16) U32 sum |x w| + U32 |z| (the spare units
    as in gemm_acc_bound); the activation as in gemm_form (slope <= 1.2 and 16 units; ReLU is exact with slope 1); the
    residual add U32 |ref|.
    losses: drop4 (the last 4 K columns: one lane's 16-byte load), odd_wave (the chunks of the odd wave of the pair; K > 1024),
    act_after_resid, resid_row0 (the residual of row 0 for every row), ldx_ignored (x rows read at stride K)."""
    N, K = W.shape
    stride = K if loss == "ldx_ignored" else ldx
    x = torch.stack([xbuf.reshape(-1)[b * stride: b * stride + K] for b in range(B)])
    if loss == "resid_row0":
        resid = resid[:1].expand(B, N)
    if emulate:
        assert loss is None
        return _gemv_skinny_emulate(x.float(), W.float(), bias, resid, act)
    x64, W64 = x.double(), W.double()
    if loss == "drop4":
        W64 = W64.clone()
        W64[:, K - 4:] = 0
    if loss == "odd_wave":
        assert K > GEMV_CH
        W64 = W64.clone()
        for c in range(1, (K + GEMV_CH - 1) // GEMV_CH, 2):
            W64[:, c * GEMV_CH:(c + 1) * GEMV_CH] = 0
    z = x64 @ W64.T
    ez = (K / 64 + 16) * U32 * (x.double().abs() @ W.double().abs().T)
    if bias is not None:
        z = z + bias.double()
    ez = ez + U32 * z.abs()
    if loss == "act_after_resid":
        return G._ACTS[act](z + resid.double()), None
    c = G._ACTS[act](z)
    e = ez if act in (ACT_NONE, ACT_RELU) else 1.2 * ez + 16 * U32 * c.abs()
    if resid is not None:
        c = c + resid.double()
        e = e + U32 * c.abs()
    return c, e


def _gemv_skinny_emulate(x, W, bias, resid, act):
    """the lane chains of the kernel: wave `half` of a pair takes chunks 2 ci + half; in a chunk lane l multiplies columns
    c * 1024 + u * 256 + 4 l + i (u = 0 .. 3, i = 0 .. 3) by FMA into one sum per (row, batch row); xor butterfly; the even
    wave adds the odd wave's sum; bias, activation, residual"""
    B, K = x.shape
    N = W.shape[0]
    nch = (K + GEMV_CH - 1) // GEMV_CH
    nchp = (nch + 1) // 2
    lane = torch.arange(64)
    acc = torch.zeros(2, B, N, 64)
    for half in range(2):
        a = torch.zeros(B, N, 64)
        for ci in range(nchp):
            c = 2 * ci + half
            if c >= nch:
                continue
            for u in range(4):
                k0 = c * GEMV_CH + u * 256 + lane * 4
                live = k0 < K                      # K % 4 == 0: a lane's four columns are in or out together
                kk = torch.where(live, k0, torch.zeros_like(k0))
                for i in range(4):
                    w = torch.where(live, W[:, kk + i], torch.zeros(()))          # [N, 64]
                    xv = torch.where(live, x[:, kk + i], torch.zeros(()))         # [B, 64]
                    a = _fma(a, w[None], xv[:, None])
        acc[half] = _butterfly(a)
    z = (acc[0] + acc[1])[..., 0]
    if bias is not None:
        z = z + bias.float()
    y = G._ACTS[act](z)
    if resid is not None:
        y = y + resid.float()
    return y


# =====================================================================================================================
# mask-decoder tails
# =====================================================================================================================
def _unshuffle(tmp, n, g, C, swapped=False):
    """tmp [n*g*g, 4*C] (col = (dy*2 + dx)*C + c) -> [n, 2g, 2g, C]: src = tmp[i, Y/2, X/2, ((Y&1)*2 + (X&1))*C : +C]"""
    t = tmp.reshape(n, g, g, 2, 2, C)                    # [i, y, x, dy, dx, c]
    if swapped:                                          # (X&1)*2 + (Y&1): dy and dx exchanged
        t = t.transpose(3, 4)
    return t.permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * g, 2 * g, C)


def upscale1(tmp, n, g, C, gain, bias, eps, *, loss=None, emulate=False):
    """out [n*2g*2g, C] f32 = gelu(LayerNorm2d over C of the un-shuffled ConvT output): norm_form with act = GELU and an f32
    output, on the rows the un-shuffle produces.
    losses: parity_swapped, no_eps, act_dropped (norm_form's), second_half_mean (C > 64: the second value per lane left out
    of the mean)"""
    src = _unshuffle(tmp, n, g, C, swapped=(loss == "parity_swapped")).reshape(-1, C)
    if loss == "second_half_mean":
        assert C > 64
        x, gn, b = src.double(), gain.double(), bias.double()
        d = x - x[:, :64].sum(-1, keepdim=True) / C
        rs = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
        return torch.nn.functional.gelu(gn * d * rs + b), None
    nl = loss if loss in ("no_eps", "act_dropped") else None
    return norm_form(0, src, gain, bias, eps, act=ACT_GELU, y_f32=True, loss=nl, emulate=emulate)


def upscale2_masks(tmp, hyper, n, ntok, g2, C, *, loss=None, emulate=False):
    """masks [n, ntok, 2 g2, 2 g2]: u = gelu(v) on the un-shuffled v, ref[i, t, Y, X] = sum_c hyper[i, t, c] u_c.
    bound: C FMAs in one chain + 2 spare: (C + 2) U32 sum |hyper u|; the f32 GELU itself: 16 U32 (|u| + |v|) per channel
    weighted by |hyper| -- the |v| term is erff's ABSOLUTE error through 0.5 v (1 + erf), whose sum cancels for negative v so
    that an error relative to u would not cover it; 16 units is the project's figure for an f32 activation.
    losses: parity_swapped, hyper_prompt0 (n >= 2), gelu_missing_last (no GELU on channel C - 1)"""
    v = _unshuffle(tmp, n, g2, C, swapped=(loss == "parity_swapped"))            # [n, G, G, C]
    h = hyper.reshape(n, ntok, C)
    if loss == "hyper_prompt0":
        assert n >= 2
        h = h[:1].expand(n, ntok, C)
    if emulate:
        assert loss is None
        v, h = v.float(), h.float()
        u = torch.nn.functional.gelu(v)
        acc = torch.zeros(n, ntok, 2 * g2, 2 * g2)
        for c in range(C):
            acc = _fma(acc, h[:, :, None, None, c], u[:, None, :, :, c])
        return acc
    v, h = v.double(), h.double()
    u = torch.nn.functional.gelu(v)
    if loss == "gelu_missing_last":
        u = u.clone()
        u[..., C - 1] = v[..., C - 1]
    ref = torch.einsum("itc,iyxc->ityx", h, u)
    v0 = _unshuffle(tmp, n, g2, C).double()               # the bound is the true operands' whatever the loss
    u0, h0 = torch.nn.functional.gelu(v0).abs(), hyper.reshape(n, ntok, C).double().abs()
    bound = (C + 2) * U32 * torch.einsum("itc,iyxc->ityx", h0, u0) + \
        16 * U32 * torch.einsum("itc,iyxc->ityx", h0, u0 + v0.abs())
    return ref, bound


def dense_pe(gauss, g, F, *, loss=None, emulate=False):
    """out [g*g, 2F]: c = 2 (i + 1/2) / g - 1, v = 2 pi (c_x G0 + c_y G1), out = sin v | cos v.
    bound: the argument is off by dv = 2 pi U32 (8 (|c_x G0| + |c_y G1|) + 2 (|G0| + |G1|)) -- c itself is within 2 U32
    (one division, one multiply by 2, one subtraction of values <= 2) which moves a product by 2 U32 |G|; the two products, the
    sum, the multiply by the f32 constant 2 pi (itself off by < U32 relative) and spare: 8 units of the products; |sin'|,
    |cos'| <= 1.  sinf / cosf: 4 ulp of a value <= 1 = 4 U32, the OpenCL full-profile limit (no math-accuracy table ships
    with the ROCm installation this was written against, so no larger documented figure replaces it).
    losses: no_half_pixel, xy_swapped, sincos_swapped"""
    f = (lambda t: t.float()) if emulate else (lambda t: t.double())
    i = f(torch.arange(g))
    off = 0.0 if loss == "no_half_pixel" else 0.5
    if emulate:
        c = 2.0 * ((i + 0.5) / torch.tensor(float(g))) - 1.0
    else:
        c = 2.0 * (i + off) / g - 1.0
    G0, G1 = f(gauss[0]), f(gauss[1])
    cx, cy = c[None, :, None], c[:, None, None]             # out row = y * g + x
    if loss == "xy_swapped":
        cx, cy = cy, cx
    a, b = cx * G0, cy * G1
    if emulate:
        v = torch.tensor(6.283185307179586, dtype=torch.float32) * (a + b)
        return torch.cat([torch.sin(v), torch.cos(v)], -1).reshape(g * g, 2 * F)
    v = 2 * math.pi * (a + b)
    s, co = torch.sin(v), torch.cos(v)
    if loss == "sincos_swapped":
        s, co = co, s
    ref = torch.cat([s, co], -1).reshape(g * g, 2 * F)
    dv = 2 * math.pi * U32 * (8 * (a.abs() + b.abs()) + 2 * (G0.abs() + G1.abs()))
    bound = (dv + 4 * U32).repeat(1, 1, 2).reshape(g * g, 2 * F)
    return ref, bound


def l2norm_scale(x, scale, *, loss=None, emulate=False):
    """y = x / max(||x||, 1e-12) * scale, one 256-thread workgroup per row.
    bound ((ceil(D / 256) + 9) / 2 + 4) U32 |ref|: the sum of squares is a chain of ceil(D / 256) products-and-adds per thread,
    6 butterfly levels and 3 adds of the four waves (+ 9), all relative to a sum of positive terms and HALVED by the square
    root; then sqrtf, the division, the multiply and one spare (4).  A zero row has a zero bound: exact zeros.
    losses: last_dropped (the last element left out of the norm)"""
    rows, D = x.shape
    if emulate:
        assert loss is None
        x = x.float()
        pad = (-D) % 256
        xp = torch.cat([x, torch.zeros(rows, pad)], 1).reshape(rows, -1, 256)      # element d belongs to thread d % 256
        ss = torch.zeros(rows, 256)
        for j in range(xp.shape[1]):
            ss = ss + xp[:, j] * xp[:, j]
        w = _butterfly(ss.reshape(rows, 4, 64))[..., 0]                              # red[0 .. 3]
        tot = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        nrm = torch.sqrt(tot).clamp_min(1e-12)[:, None]
        return x / nrm * torch.tensor(scale, dtype=torch.float32)
    x = x.double()
    xs = x[:, :-1] if loss == "last_dropped" else x
    nrm = xs.norm(dim=1, keepdim=True).clamp_min(1e-12)
    ref = x / nrm * float(torch.tensor(scale, dtype=torch.float32))
    bound = ((math.ceil(D / 256) + 9) / 2 + 4) * U32 * ref.abs()
    return ref, bound


# =====================================================================================================================
# exact kernels.  Every function returns the f32 VALUES the output holds (16-bit outputs: exactly representable, the test
# converts with .to(dtype) and compares the 16-bit words).  emulate=True: the kernel's flat-index arithmetic.
# =====================================================================================================================
def build_tokens(out_tokens, pred, *, emulate=False):
    """tokens [n, n_out + 1, C]: rows 0 .. n_out - 1 = out_tokens, row n_out = pred[i]"""
    n_out, C = out_tokens.shape
    n = pred.shape[0]
    if emulate:
        t = torch.arange(n_out + 1)[None, :].expand(n, -1)
        i = torch.arange(n)[:, None].expand(-1, n_out + 1)
        src = torch.cat([out_tokens.reshape(-1), pred.reshape(-1)])
        base = torch.where(t < n_out, t * C, n_out * C + i * C)
        return src[base[..., None] + torch.arange(C)]
    return torch.cat([out_tokens[None].expand(n, -1, -1), pred[:, None]], 1).contiguous()


def add_rows(a, b, bmod, *, loss=None, emulate=False):
    """out[m] = a[m] + b[m % bmod]: one IEEE f32 add.  losses: bmod_ignored (b[m], the last row of b past its end)"""
    M, D = a.shape
    if emulate:
        i = torch.arange(M * D)
        m, d = i // D, i % D
        return (a.reshape(-1)[i] + b.reshape(-1)[(m % bmod) * D + d]).reshape(M, D)
    m = torch.arange(M)
    idx = m.clamp_max(bmod - 1) if loss == "bmod_ignored" else m % bmod
    return a.float() + b.float()[idx]


def add_vec(a, v, *, emulate=False):
    if emulate:
        i = torch.arange(a.numel())
        return (a.reshape(-1)[i] + v[i % a.shape[1]]).reshape(a.shape)
    return a.float() + v.float()[None]


def clip_assemble(patch, cls, pos, rows, x0, *, loss=None, emulate=False):
    """x [B, rows, D] (rows = 0: n + 1): x[b, 0] = cls + pos[0], x[b, 1 + i] = patch[b, i] + pos[1 + i], spare rows zero.
    losses: pos_off_by_one (patch i takes pos[i]), spare_kept (rows past n + 1 keep x0)"""
    B, n, D = patch.shape
    R = rows if rows > 0 else n + 1
    if emulate:
        i = torch.arange(B * R * D)
        d, t, b = i % D, (i // D) % R, i // (D * R)
        tt = t.clamp_max(n)
        v = torch.where(tt == 0, cls[d], patch.reshape(-1)[((b * n + (tt - 1).clamp_min(0)) * D + d)])
        return torch.where(t > n, torch.zeros(()), v + pos.reshape(-1)[tt * D + d]).reshape(B, R, D)
    out = torch.zeros(B, R, D) if loss != "spare_kept" else x0.reshape(B, R, D).clone()
    out[:, 0] = cls + pos[0]
    out[:, 1:n + 1] = patch + (pos[:n] if loss == "pos_off_by_one" else pos[1:n + 1])[None]
    return out


def to_f32(src):
    """a widening: every bf16 / f16 value is an f32 value"""
    return src.float()


def dequant_fp8(q_u8, scale):
    """bf16_rne(f32(e4m3) * scale[n]); the statement is anyref_amd.quant.dequantize_rows_fp8"""
    from anyref_amd.quant import dequantize_rows_fp8
    return dequantize_rows_fp8(q_u8, scale).to(torch.bfloat16).float()


def dequant_fp8_emulate(q_u8, scale):
    """16 values per step from a table of the 256 e4m3fn codes built from the format's definition (bias 7, no infinities)"""
    code = torch.arange(256)
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    val = torch.where(e == 0, m.double() / 8 * 2.0 ** -6, (1 + m.double() / 8) * 2.0 ** (e.double() - 7))
    val = torch.where((e == 15) & (m == 7), torch.full_like(val, float("nan")), val)
    val = (torch.where(s == 1, -val, val)).float()
    return (val[q_u8.long()] * scale.float()[:, None]).to(torch.bfloat16).float()


def table_rows(table, ids):
    """rows of an embedding table widened to f32"""
    return table[ids.long()].float()


def embed_rows(ids, table):
    return table_rows(table, ids)


def gather_rows(x, b, pos, *, emulate=False):
    """out[i] = x[b[i], pos[i]] (x [B, Smax, D])"""
    if emulate:
        Smax, D = x.shape[1:]
        return x.reshape(-1, D)[b.long() * Smax + pos.long()].clone()
    return x[b.long(), pos.long()].clone()


def scatter_rows(rows, db, dp, x0, *, emulate=False):
    """x[db[i], dp[i]] = rows[i], everything else as it was; destinations distinct"""
    out = x0.clone()
    if emulate:
        Smax, D = x0.shape[1:]
        flat = out.reshape(-1, D)
        for i in range(rows.shape[0]):
            flat[int(db[i]) * Smax + int(dp[i])] = rows[i]
        return flat.reshape(x0.shape)
    out[db.long(), dp.long()] = rows
    return out


def embed_splice(ids, lens, table, vocab, img_feat, x0, *, loss=None, emulate=False):
    """x [B, Smax, D] and out_len [B].  Per row: ip = index of the FIRST -200 among the first lens[b] ids (none: plain rows).
    With an image S = L + n_img - 1: rows < ip are text rows, ip .. ip + n_img - 1 the image rows of batch b, the rest the text
    at srow - n_img + 1.  A text id < 0 or >= vocab gives a zero row; rows >= min(S, grid) keep x0, the grid being
    min(Lmax + n_img, Smax) rows.
    losses: tpos_off (text behind the image read at srow - n_img), img_batch0 (image rows of batch 0 for every batch)"""
    B, Lmax = ids.shape
    n_img = img_feat.shape[1]
    Smax, D = x0.shape[1:]
    grid = min(Lmax + n_img, Smax)
    out = x0.float().clone()
    out_len = torch.zeros(B, dtype=torch.int32)
    tab = table.float()
    if emulate:      # one pass per (b, srow) block, as the kernel's grid walks them
        for b in range(B):
            L = int(lens[b])
            ip = -1
            for i in range(L):
                if int(ids[b, i]) == -200:
                    ip = i
                    break
            S = L + n_img - 1 if ip >= 0 else L
            out_len[b] = S
            for srow in range(grid):
                if srow >= S:
                    continue
                if ip >= 0 and ip <= srow < ip + n_img:
                    out[b, srow] = img_feat[b, srow - ip]
                    continue
                tpos = srow - n_img + 1 if (ip >= 0 and srow >= ip + n_img) else srow
                tid = int(ids[b, tpos])
                out[b, srow] = tab[tid] if 0 <= tid < vocab else 0.0
        return out, out_len
    for b in range(B):
        L = int(lens[b])
        row = ids[b, :L]
        hit = (row == -200).nonzero()
        txt = torch.where(((row >= 0) & (row < vocab))[:, None], tab[row.clamp(0, vocab - 1)], torch.zeros(()))
        if hit.numel() == 0:
            seq = txt
        else:
            ip = int(hit[0])
            img = img_feat[0 if loss == "img_batch0" else b].float()
            after = txt[ip + 1:]
            if loss == "tpos_off":          # srow - n_img: one id early, starting with the placeholder itself (a zero row)
                after = txt[ip:L - 1]
            seq = torch.cat([txt[:ip], img, after])
        S = seq.shape[0]
        out_len[b] = S
        out[b, :min(S, grid)] = seq[:min(S, grid)]
    return out, out_len


def im2col_patch(img, p, Kp, ty, *, loss=None, emulate=False, out0=None):
    """img f32 [B, 3, S, S] -> [B * g * g, Kp] in type ty, k = c p^2 + ky p + kx, columns >= 3 p^2 zero.
    losses: kykx_swapped, tap_major (k = (ky p + kx) 3 + c), pad_kept (the pad columns keep out0; Kp > 3 p^2)"""
    B, _, S, _ = img.shape
    g, K = S // p, 3 * p * p
    if emulate:
        i = torch.arange(B * g * g * Kp)
        k, row = i % Kp, i // Kp
        px, py, b = row % g, (row // g) % g, row // (g * g)
        kk = k.clamp_max(K - 1)
        kx, ky, c = kk % p, (kk // p) % p, kk // (p * p)
        v = img.reshape(-1)[((b * 3 + c) * S + (py * p + ky)) * S + px * p + kx]
        return store(torch.where(k < K, v, torch.zeros(())).reshape(-1, Kp), ty)
    t = img.reshape(B, 3, g, p, g, p)                    # [b, c, py, ky, px, kx]
    if loss == "kykx_swapped":
        m = t.permute(0, 2, 4, 1, 5, 3)                  # [b, py, px, c, kx, ky]: column ky p + kx holds pixel (kx, ky)
    elif loss == "tap_major":
        m = t.permute(0, 2, 4, 3, 5, 1)                  # [b, py, px, ky, kx, c]
    else:
        m = t.permute(0, 2, 4, 1, 3, 5)                  # [b, py, px, c, ky, kx]
    out = torch.zeros(B * g * g, Kp)
    if loss == "pad_kept":
        assert Kp > K
        out = out0.float().clone()
    out[:, :K] = m.reshape(B * g * g, K)
    return store(out, ty) if loss != "pad_kept" else torch.cat([store(out[:, :K], ty), out[:, K:]], 1)


def im2col_3x3(x, ty, *, loss=None, emulate=False):
    """x f32 [B, g, g, C] as stored in type ty (pairs: both terms travel raw, so the output is the 3 x 3 gather of the
    ROUND-TRIPPED input) -> [B * g * g, 9 C], k = (ky 3 + kx) C + c, zero outside the image.
    losses: border_kept (a tap outside reads the clamped pixel instead of zero), tap_transposed (tap = kx 3 + ky)"""
    B, g, _, C = x.shape
    xs = store(x, ty)
    if emulate:
        i = torch.arange(B * g * g * 9 * C)
        c, tap, row = i % C, (i // C) % 9, i // (9 * C)
        xx0, yy0, b = row % g, (row // g) % g, row // (g * g)
        yy, xx = yy0 + tap // 3 - 1, xx0 + tap % 3 - 1
        inside = (yy >= 0) & (yy < g) & (xx >= 0) & (xx < g)
        v = xs.reshape(-1)[((b * g + yy.clamp(0, g - 1)) * g + xx.clamp(0, g - 1)) * C + c]
        return torch.where(inside, v, torch.zeros(())).reshape(-1, 9 * C)
    taps = []
    for tap in range(9):
        dy, dx = (tap % 3 - 1, tap // 3 - 1) if loss == "tap_transposed" else (tap // 3 - 1, tap % 3 - 1)
        ys, xs_ = torch.arange(g) + dy, torch.arange(g) + dx
        v = xs[:, ys.clamp(0, g - 1)][:, :, xs_.clamp(0, g - 1)]
        if loss != "border_kept":
            ok = ((ys >= 0) & (ys < g))[:, None] & ((xs_ >= 0) & (xs_ < g))[None, :]
            v = torch.where(ok[None, :, :, None], v, torch.zeros(()))
        taps.append(v)
    return torch.stack(taps, 3).reshape(B * g * g, 9 * C)


def im2col_conv1(img, k, st, ty, *, loss=None, emulate=False):
    """img f32 [n, Hh, Ww] -> [n * gh * gw, k * k] in type ty, gh = (Hh - k) / st + 1: patches overlap (st < k).
    losses: stride_k (the patch origin advances by k instead of st; origins clamped to the image)"""
    n, Hh, Ww = img.shape
    gh, gw = (Hh - k) // st + 1, (Ww - k) // st + 1
    if emulate:
        i = torch.arange(n * gh * gw * k * k)
        e, row = i % (k * k), i // (k * k)
        px, py, b = row % gw, (row // gw) % gh, row // (gh * gw)
        return store(img.reshape(-1)[(b * Hh + py * st + e // k) * Ww + px * st + e % k].reshape(-1, k * k), ty)
    step = k if loss == "stride_k" else st
    oy = (torch.arange(gh) * step).clamp_max(Hh - k)
    ox = (torch.arange(gw) * step).clamp_max(Ww - k)
    ey = oy[:, None] + torch.arange(k)[None]             # [gh, k]
    ex = ox[:, None] + torch.arange(k)[None]             # [gw, k]
    m = img[:, ey][:, :, :, ex]                          # [n, gh, k, gw, k]
    return store(m.permute(0, 1, 3, 2, 4).reshape(n * gh * gw, k * k), ty)


# =====================================================================================================================
# cases and operands shared by the CPU proof and the GPU tests.  Every *_case returns a dict of CPU tensors: the operands,
# "ref" (bounded kernels: and "bound") and "mutants" {name: tensor}.
# =====================================================================================================================
def _gen(*key):
    """a generator seeded by the case's numbers (the same stream in the CPU proof and on the card)"""
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# (B, N, K, ldx, act, resid, ldy, bias): resid "alias" = the residual is y itself, "own" = a buffer of its own, None
GEMV_CASES = [
    (1, 4, 256, 7 * 256, ACT_RELU, None, 4, True),          # the iou head: x rows NQ * C apart, N = 4, ldy = N
    (6, 256, 256, 256, ACT_NONE, "alias", 259, True),       # NB = 8 with nb = 6
    (3, 128, 256, 260, ACT_NONE, "own", 131, True),         # NB = 4 with nb = 3, ldx != K
    (7, 2048, 256, 256, ACT_RELU, None, 2051, True),
    (7, 256, 2048, 2048, ACT_NONE, "alias", 259, True),     # two chunks, one per half of the wave pair
    (2, 33, 36, 40, ACT_NONE, "own", 36, True),             # less than one load row per lane, odd N, ldx != K
    (4, 10, 3076, 3076, ACT_NONE, None, 13, False),         # four chunks, the last one ragged (4 columns: one lane), no bias
    (4, 10, 2052, 2052, ACT_NONE, "own", 13, True),         # an ODD chunk count (3): the odd wave has a dead slot
    (1, 256, 4096, 4096, ACT_RELU, None, 259, True),
    (8, 4096, 4096, 4096, ACT_RELU, None, 4099, True),      # 128 KB of LDS, 2048 groups, the 512-workgroup cap
    (5, 4100, 4096, 4096, ACT_NONE, "alias", 4103, True),   # 2050 groups on 2048 wave pairs: a second, mostly dead pass
] + [(2, 64, 256, 256, act, "own", 67, True) for act in range(5)]
GEMV_REFUSED = [(9, 64, 256, 256), (2, 64, 4100, 4100), (2, 64, 258, 258), (2, 64, 256, 257)]     # (B, N, K, ldx)


def gemv_case(B, N, K, ldx, act, resid, ldy, with_bias):
    g = _gen(B, N, K, ldx, act)
    xbuf = torch.randn(max(B, 2) * ldx, generator=g)         # (a second row's worth even at B = 1: the stride stays visible)
    W = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g) * 0.5 if with_bias else None
    r = torch.randn(B, N, generator=g) if resid else None
    ref, bound = gemv_skinny(xbuf, ldx, W, bias, r, act, B)
    losses = ["drop4"] + (["odd_wave"] if K > GEMV_CH else []) + \
        (["act_after_resid"] if (act != ACT_NONE and resid) else []) + (["resid_row0"] if (B >= 2 and resid) else []) + \
        (["ldx_ignored"] if (B >= 2 and ldx != K) else [])
    muts = {n: gemv_skinny(xbuf, ldx, W, bias, r, act, B, loss=n)[0] for n in losses}
    return dict(xbuf=xbuf, W=W, bias=bias, resid=r, ref=ref, bound=bound, mutants=muts)


UPSCALE1_CASES = [(2, 3, 64), (3, 2, 32), (1, 2, 128), (1, 3, 100), (1, 1, 5)]       # (n, g, C); C > 64: the second lane value
UPSCALE1_EPS = 1e-6


def upscale1_case(n, g, C):
    gen = _gen(n, g, C, 1)
    tmp = torch.randn(n * g * g, 4 * C, generator=gen) * 2 + 0.5
    tmp[::3] *= 1e-3 / 2          # pixels whose deviation is ~ sqrt(eps): without eps they are off by tens of per cent
    gain, bias = 1 + 0.2 * torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    ref, bound = upscale1(tmp, n, g, C, gain, bias, UPSCALE1_EPS)
    losses = ["parity_swapped", "no_eps", "act_dropped"] + (["second_half_mean"] if C > 64 else [])
    muts = {k: upscale1(tmp, n, g, C, gain, bias, UPSCALE1_EPS, loss=k)[0] for k in losses}
    return dict(tmp=tmp, gain=gain, bias=bias, ref=ref, bound=bound, mutants=muts)


UPSCALE2_CASES = [(2, 4, 3, 32), (1, 8, 9, 5), (2, 1, 2, 64)]       # (n, ntok, g2, C); g2 = 9: 324 pixels, a ragged second block


def upscale2_case(n, ntok, g2, C):
    gen = _gen(n, ntok, g2, C, 2)
    tmp = torch.randn(n * g2 * g2, 4 * C, generator=gen) * 1.5
    hyper = torch.randn(n, ntok, C, generator=gen)
    ref, bound = upscale2_masks(tmp, hyper, n, ntok, g2, C)
    losses = ["parity_swapped", "gelu_missing_last"] + (["hyper_prompt0"] if n >= 2 else [])
    muts = {k: upscale2_masks(tmp, hyper, n, ntok, g2, C, loss=k)[0] for k in losses}
    return dict(tmp=tmp, hyper=hyper, ref=ref, bound=bound, mutants=muts)


DENSE_PE_CASES = [(14, 128), (5, 3), (64, 128)]


def dense_pe_case(g, F):
    gauss = torch.randn(2, F, generator=_gen(g, F, 3))
    ref, bound = dense_pe(gauss, g, F)
    muts = {k: dense_pe(gauss, g, F, loss=k)[0] for k in ("no_half_pixel", "xy_swapped", "sincos_swapped")}
    return dict(gauss=gauss, ref=ref, bound=bound, mutants=muts)


L2NORM_CASES = [(3, 1024), (2, 5), (2, 300)]
L2NORM_SCALE = 20.0


def l2norm_case(rows, D):
    x = torch.randn(rows, D, generator=_gen(rows, D, 4)) * 3
    x[0] = 0
    ref, bound = l2norm_scale(x, L2NORM_SCALE)
    return dict(x=x, ref=ref, bound=bound, mutants={"last_dropped": l2norm_scale(x, L2NORM_SCALE, loss="last_dropped")[0]})


TABLE_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
SPLICE_CASES = [(D, dt, Smax) for D in (40, 300) for dt in (0, 1, 2) for Smax in (17, 16)]
SPLICE_B, SPLICE_LMAX, SPLICE_NIMG, SPLICE_VOCAB = 4, 12, 5, 50


def splice_case(D, dt, Smax):
    B, Lmax, n_img, vocab = SPLICE_B, SPLICE_LMAX, SPLICE_NIMG, SPLICE_VOCAB
    gen = _gen(D, dt, Smax, 5)
    ids = torch.randint(0, vocab, (B, Lmax), generator=gen)
    lens = torch.tensor([12, 7, 3, 8], dtype=torch.int32)
    ids[0, 5] = -200                 # placeholder in the middle of a full-length row ...
    ids[0, 9] = -200                 # ... a second one is a foreign placeholder: a zero row
    ids[2, :3] = torch.tensor([-200, -300, vocab])       # placeholder first, L = 3, a foreign id and one past the table
    ids[3, 7] = -200                 # placeholder last
    ids[1, 9] = -200                 # behind lens[1]: not a placeholder of this row
    table = torch.randn(vocab, D, generator=gen).to(TABLE_DT[dt])
    img = torch.randn(B, n_img, D, generator=gen)
    x0 = nan_fill((B, Smax, D))
    ref, out_len = embed_splice(ids, lens, table, vocab, img, x0)
    muts = {k: embed_splice(ids, lens, table, vocab, img, x0, loss=k)[0] for k in ("tpos_off", "img_batch0")}
    return dict(ids=ids, lens=lens, table=table, img=img, x0=x0, ref=ref, out_len=out_len, mutants=muts)


ROWS_CASES = [(D, n) for D in (40, 300) for n in (1, 5)]


def rows_case(D, n):
    """gather / scatter / embed_rows / build_tokens operands: repeated and out-of-order indices (scatter: distinct ones)"""
    gen = _gen(D, n, 6)
    Bx, Smax, vocab = 3, 6, 11
    x = torch.randn(Bx, Smax, D, generator=gen)
    gb = torch.tensor([2, 0, 2, 1, 0][:n], dtype=torch.int32)
    gp = torch.tensor([5, 3, 5, 0, 1][:n], dtype=torch.int32)             # (2, 5) twice, batches out of order
    sb = torch.tensor([2, 0, 1, 2, 0][:n], dtype=torch.int32)
    sp = torch.tensor([4, 5, 0, 1, 2][:n], dtype=torch.int32)             # distinct destinations, out of order
    rows = torch.randn(n, D, generator=gen)
    ids = torch.tensor([7, 0, 7, 10, 3][:n], dtype=torch.int64)
    table = torch.randn(vocab, D, generator=gen)
    out_tokens, pred = torch.randn(5, D, generator=gen), torch.randn(n, D, generator=gen)
    return dict(x=x, gb=gb, gp=gp, sb=sb, sp=sp, rows=rows, ids=ids, table=table, out_tokens=out_tokens, pred=pred)


# (B, S, p, Kp, types)
PATCH_CASES = [(2, 28, 14, 588, (0, 1, 2)), (2, 28, 14, 640, (0, 1, 2, 3, 4)), (1, 32, 16, 768, (0, 1, 2, 3, 4))]
C3X3_CASES = [(2, 3, 64, (0, 1, 2, 3, 4)), (1, 1, 64, (0, 1, 2, 3, 4)), (1, 5, 24, (0, 1, 2))]                 # (B, g, C, types)
CONV1_CASES = [(2, 36, 46, 16, 10, (0, 1, 2, 3, 4)), (1, 8, 9, 4, 3, (0, 1, 2))]                             # (n, Hh, Ww, k, st, types)


def flat(cases):
    return [c[:-1] + (t,) for c in cases for t in c[-1]]


def patch_case(B, S, p, Kp, ty):
    img = torch.randn(B, 3, S, S, generator=_gen(B, S, p, Kp, 7))
    rows = B * (S // p) ** 2
    out0 = nan_fill((rows, Kp))
    losses = ["kykx_swapped", "tap_major"] + (["pad_kept"] if Kp > 3 * p * p else [])
    muts = {k: im2col_patch(img, p, Kp, ty, loss=k, out0=out0) for k in losses}
    return dict(img=img, ref=im2col_patch(img, p, Kp, ty), mutants=muts)


def c3x3_case(B, g, C, ty):
    x = torch.randn(B, g, g, C, generator=_gen(B, g, C, 8))
    losses = ["border_kept"] + (["tap_transposed"] if g > 1 else [])     # g = 1: the centre tap is its own transpose
    return dict(x=x, ref=im2col_3x3(x, ty), mutants={k: im2col_3x3(x, ty, loss=k) for k in losses})


def conv1_case(n, Hh, Ww, k, st, ty):
    img = torch.randn(n, Hh, Ww, generator=_gen(n, Hh, Ww, k, st, 9))
    return dict(img=img, ref=im2col_conv1(img, k, st, ty), mutants={"stride_k": im2col_conv1(img, k, st, ty, loss="stride_k")})


CLIP_CASES = [(2, 4, 40, 0), (3, 4, 300, 6)]           # (B, n, D, rows)


def clip_case(B, n, D, rows):
    gen = _gen(B, n, D, rows, 10)
    patch, cls, pos = torch.randn(B, n, D, generator=gen), torch.randn(D, generator=gen), torch.randn(n + 1, D, generator=gen)
    R = rows if rows > 0 else n + 1
    x0 = nan_fill((B, R, D))
    losses = ["pos_off_by_one"] + (["spare_kept"] if R > n + 1 else [])
    muts = {k: clip_assemble(patch, cls, pos, rows, x0, loss=k) for k in losses}
    return dict(patch=patch, cls=cls, pos=pos, x0=x0, ref=clip_assemble(patch, cls, pos, rows, x0), mutants=muts)


ADD_ROWS_CASES = [(6, 40, 6), (12, 300, 3)]            # (M, D, bmod)


def add_rows_case(M, D, bmod):
    gen = _gen(M, D, bmod, 11)
    a, b, v = torch.randn(M, D, generator=gen), torch.randn(bmod, D, generator=gen), torch.randn(D, generator=gen)
    muts = {"bmod_ignored": add_rows(a, b, bmod, loss="bmod_ignored")} if bmod < M else {}     # bmod = M: the same rows
    return dict(a=a, b=b, v=v, ref=add_rows(a, b, bmod), ref_vec=add_vec(a, v), mutants=muts)


DEQUANT_CASES = [(3, 48), (5, 688)]                    # (N, K)


def dequant_case(N, K):
    gen = _gen(N, K, 12)
    q = torch.randint(0, 256, (N, K), generator=gen).to(torch.uint8)
    q[(q & 0x7F) == 0x7F] = 0x38        # the two NaN codes of e4m3fn never leave the quantiser
    scale = torch.rand(N, generator=gen) * 0.02 + 1e-3
    return dict(q=q, scale=scale, ref=dequant_fp8(q, scale))
