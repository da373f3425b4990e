"""Float64 references, derived per-element bounds and mutants for the two spatial-prompt kernels (anyref_amd/csrc/prompt_encode.hip):
prompt_tokens (the decoder's token matrix with point / box / text rows) and mask_prompt_embed (the fused mask_downscaling that
writes the decoder's keys).  tests/test_gpu_prompt_ops.py runs the kernels against them through the anyref_op_* entry points;
tests/test_cpu_prompt_ops_ref.py proves on the CPU that every bound admits an f32 emulation in the kernel's order and rejects
every mutant.  Conventions and helpers: tests/glue_ops_ref.py (the reference is float64 over the operands AS STORED, a bound is
a sum of terms each written down where it is added, none is tuned to what a kernel returns, a mutant is the reference with one
plausible loss).
"""
import math

import torch

import glue_ops_ref as R
from glue_ops_ref import U32, norm_form, ACT_GELU, _fma, _gen

TWO_PI_F32 = torch.tensor(6.283185307179586, dtype=torch.float32)
LN_EPS = 1e-6


# =====================================================================================================================
# prompt_tokens
# =====================================================================================================================
TOKEN_LOSSES = ("no_half_pixel", "xy_swapped", "sincos_swapped", "pad_missing", "pad_with_box", "label01_swapped",
                "corners_swapped", "nap_keeps_pe", "text_first")


def _pe(xy, gauss, S, *, loss=None, emulate=False):
    """xy [..., 2] pixels -> (sin v | cos v [..., C], bound): c = 2 ((p + 1/2) / S) - 1, v = 2 pi (c_x G0 + c_y G1).
    bound: dense_pe's argument term with one more rounding in c (the p + 1/2 add): c is within 3 U32 of values <= 2, which
    moves a product by 3 U32 |G|; the two products, the sum, the multiply by the f32 2 pi and spare: 8 units of the products;
    |sin'|, |cos'| <= 1.  sinf / cosf: 4 U32 (glue_ops_ref.dense_pe)."""
    F = gauss.shape[1]
    if loss == "xy_swapped":
        xy = xy.flip(-1)
    if emulate:
        xy, G = xy.float(), gauss.float()
        Sf = torch.tensor(float(S))
        cx, cy = 2.0 * ((xy[..., 0:1] + 0.5) / Sf) - 1.0, 2.0 * ((xy[..., 1:2] + 0.5) / Sf) - 1.0
        v = TWO_PI_F32 * (cx * G[0] + cy * G[1])
        return torch.cat([torch.sin(v), torch.cos(v)], -1), None
    xy, G = xy.double(), gauss.double()
    off = 0.0 if loss == "no_half_pixel" else 0.5
    cx, cy = 2.0 * ((xy[..., 0:1] + off) / S) - 1.0, 2.0 * ((xy[..., 1:2] + off) / S) - 1.0
    a, b = cx * G[0], cy * G[1]
    v = 2 * math.pi * (a + b)
    s, co = torch.sin(v), torch.cos(v)
    if loss == "sincos_swapped":
        s, co = co, s
    dv = 2 * math.pi * U32 * (8 * (a.abs() + b.abs()) + 3 * (G[0].abs() + G[1].abs()))
    return torch.cat([s, co], -1), (dv + 4 * U32).repeat(*([1] * (xy.dim() - 1)), 2)


def token_rows(n_out, P, boxes, text):
    return n_out + P + (1 if P > 0 and not boxes else 0) + (2 if boxes else 0) + (1 if text else 0)


def prompt_tokens(out_tokens, points, labels, boxes, text, gauss, emb5, S, *, loss=None, emulate=False):
    """tokens [n, NQ, C]: out_tokens, the points (PE + emb5[label] for label 0 / 1, emb5[4] alone for -1, the PE alone for
    any other label), the pad (emb5[4]; iff points and no boxes), the corners (PE + emb5[2], PE + emb5[3]), text.
    bound: zero on the copied rows (out_tokens, not-a-point rows, text: bit for bit); a PE row: _pe's bound, and where an
    embedding is added one f32 add: U32 |ref|.
    A mutant that changes the row count is cut or zero-filled to the reference's rows (what the same buffer would hold)."""
    f = (lambda t: t.float()) if emulate else (lambda t: t.double())
    n_out, C = out_tokens.shape
    n = next(t.shape[0] for t in (points, boxes, text) if t is not None)
    P = 0 if points is None else points.shape[1]
    E = f(emb5)
    zero = torch.zeros(n, 1, C, dtype=E.dtype)
    rows, bounds = [f(out_tokens)[None].expand(n, -1, -1)], [zero.expand(n, n_out, C)]
    e01 = (1, 0) if loss == "label01_swapped" else (0, 1)
    e23 = (3, 2) if loss == "corners_swapped" else (2, 3)
    txt = [] if text is None else [(f(text)[:, None], zero)]
    if loss == "text_first":
        rows += [t for t, _ in txt]
        bounds += [b for _, b in txt]
    if P:
        pe, pb = _pe(points, gauss, S, loss=loss, emulate=emulate)
        lab = labels.long()[..., None]
        nap = lab == -1
        val = pe + (lab == 0) * E[e01[0]] + (lab == 1) * E[e01[1]]
        if loss == "nap_keeps_pe":
            val = torch.where(nap, pe + E[4], val)
        else:
            val = torch.where(nap, E[4].expand_as(pe), val)
        rows.append(val)
        if not emulate:
            added = (lab == 0) | (lab == 1)
            bounds.append(torch.where(nap, torch.zeros_like(pb), pb + added * U32 * val.abs()))
        pad = boxes is None
        if loss == "pad_missing":
            pad = False
        if loss == "pad_with_box":
            pad = True
        if pad:
            rows.append(E[4].expand(n, 1, C))
            bounds.append(zero)
    if boxes is not None:
        pe, pb = _pe(boxes.reshape(n, 2, 2), gauss, S, loss=loss, emulate=emulate)
        val = pe + torch.stack([E[e23[0]], E[e23[1]]])
        rows.append(val)
        if not emulate:
            bounds.append(pb + U32 * val.abs())
    if loss != "text_first":
        rows += [t for t, _ in txt]
        bounds += [b for _, b in txt]
    out = torch.cat(rows, 1)
    NQ = token_rows(n_out, P, boxes is not None, text is not None)
    if out.shape[1] != NQ:
        assert loss in ("pad_missing", "pad_with_box")
        out = torch.cat([out, torch.zeros(n, max(0, NQ - out.shape[1]), C, dtype=out.dtype)], 1)[:, :NQ]
    if emulate:
        return out.contiguous()
    return out.contiguous(), (None if loss else torch.cat(bounds, 1).contiguous())


# (n, P, box, text, C): the three shapes of the issue; every loss is applicable in at least one
TOKEN_CASES = [(1, 0, True, False, 256), (3, 3, False, True, 256), (2, 1, True, True, 64)]
TOKEN_N_OUT, TOKEN_S = 5, 224
TOKEN_REFUSED = [dict(C=12), dict(C=4), dict(n=0), dict(P=2, labels=None)]


def token_losses(n, P, box, text, C):
    out = ["no_half_pixel", "xy_swapped", "sincos_swapped"]
    if P and not box:
        out.append("pad_missing")
    if P and box:
        out.append("pad_with_box")
    if P:
        out += ["label01_swapped", "nap_keeps_pe"]
    if box:
        out.append("corners_swapped")
    if text and (P or box):
        out.append("text_first")
    return out


def token_case(n, P, box, text, C):
    g = _gen(n, P, int(box), int(text), C, 41)
    S = TOKEN_S
    out_tokens = torch.randn(TOKEN_N_OUT, C, generator=g)
    gauss = torch.randn(2, C // 2, generator=g)
    emb5 = torch.randn(5, C, generator=g) * 0.5
    points = torch.rand(n, P, 2, generator=g) * (S - 1) if P else None
    # every label value in every case with points; 2 is "any other label": the PE alone
    labels = {(3, 3): torch.tensor([[1, 0, -1], [1, 2, 0], [-1, 0, 1]], dtype=torch.int32),
              (2, 1): torch.tensor([[0], [-1]], dtype=torch.int32)}[(n, P)] if P else None
    boxes = None
    if box:
        a = torch.rand(n, 2, generator=g) * (S / 2)
        boxes = torch.cat([a, a + 1 + torch.rand(n, 2, generator=g) * (S / 2 - 1)], 1)
    txt = torch.randn(n, C, generator=g) * 0.5 if text else None
    args = (out_tokens, points, labels, boxes, txt, gauss, emb5, S)
    ref, bound = prompt_tokens(*args)
    muts = {k: prompt_tokens(*args, loss=k)[0] for k in token_losses(n, P, box, text, C)}
    return dict(out_tokens=out_tokens, points=points, labels=labels, boxes=boxes, text=txt, gauss=gauss, emb5=emb5, S=S,
                ref=ref, bound=bound, mutants=muts)


# =====================================================================================================================
# mask_prompt_embed
# =====================================================================================================================
EMBED_LOSSES = ("taps_swapped", "positions_permuted", "no_eps", "ln_wrong_axis", "gelu2_missing", "dense_prompt0",
                "emb_not_added")


def _ln_gelu(x, gain, bias, *, loss=None, emulate=False):
    """norm_form over the last axis with GELU, f32 output -> (y, bound of the f32 arithmetic on exact x), and the factor that
    carries an input error e (per element) to the output: 1.2 |g| rs (e' + |d| rs^2 mean(|d| e')), e' = e + mean(e) -- the
    form norm_form uses for its own mean error, with GELU's slope <= 1.2"""
    nl = loss if loss in ("no_eps",) else None
    if loss == "gelu2_missing":
        nl = "act_dropped"
    if emulate:
        return norm_form(0, x, gain, bias, LN_EPS, act=ACT_GELU, y_f32=True, emulate=True), None, None
    y, b = norm_form(0, x, gain, bias, LN_EPS, act=ACT_GELU, y_f32=True, loss=nl)
    x, g = x.double(), gain.double()
    d = x - x.mean(-1, keepdim=True)
    rs = torch.rsqrt((d * d).mean(-1, keepdim=True) + LN_EPS)

    def carry(e):
        ep = e + e.mean(-1, keepdim=True)
        return 1.2 * g.abs() * rs * (ep + d.abs() * rs * rs * (d.abs() * ep).mean(-1, keepdim=True))
    return y, b, carry


def mask_prompt_embed(mask, image_emb, W, g, *, loss=None, emulate=False):
    """keys [n, g*g, C] = image_emb [g*g, C] + mask_downscaling(mask [n, 4g, 4g]) as NHWC.
    W: dict w1 [c1,1,2,2] b1 g1 be1 w2 [c2,c1,2,2] b2 g2 be2 w3 [C,c2] b3.
    bound, stage by stage (every later stage carries the earlier stages' error at first order, through |w| and _ln_gelu's
    carry): conv 1: a chain of 4 FMAs on the bias, (4 + 2) U32 (|b1| + sum |w1 m|); norm 1 + GELU: norm_form's bound (its
    statistics and 16 units for the f32 activation); conv 2: (4 c1 + 2) U32 (|b2| + sum |w2 s1|); norm 2 + GELU likewise;
    conv 3: (c2 + 2) U32 (|b3| + sum |w3 s2|); the image embedding: one f32 add, U32 |ref|."""
    n, C = mask.shape[0], image_emb.shape[1]
    c1, c2 = W["w1"].shape[0], W["w2"].shape[0]
    f = (lambda t: t.float()) if emulate else (lambda t: t.double())
    m = f(mask).reshape(n, g, 2, 2, g, 2, 2).permute(0, 1, 4, 2, 5, 3, 6)          # [i, y, x, py, px, dy, dx]
    w1 = f(W["w1"]).reshape(c1, 2, 2)
    if loss == "taps_swapped":
        w1 = w1.transpose(1, 2)
    w2 = f(W["w2"])                                                                 # [c2, c1, py, px]
    if loss == "positions_permuted":
        w2 = w2.transpose(2, 3)
    w3, b1, b2, b3 = f(W["w3"]).reshape(C, c2), f(W["b1"]), f(W["b2"]), f(W["b3"])
    emb = f(image_emb).reshape(1, g, g, C)
    if emulate:
        a1 = b1.expand(n, g, g, 2, 2, c1)
        for dy in range(2):
            for dx in range(2):
                a1 = _fma(a1, w1[:, dy, dx], m[..., dy, dx, None])
        s1, _, _ = _ln_gelu(a1, W["g1"], W["be1"], emulate=True)
        a2 = b2.expand(n, g, g, c2)
        for c in range(c1):
            for py in range(2):
                for px in range(2):
                    a2 = _fma(a2, w2[:, c, py, px], s1[..., py, px, c, None])
        s2, _, _ = _ln_gelu(a2, W["g2"], W["be2"], emulate=True)
        acc = b3.expand(n, g, g, C)
        for j in range(c2):
            acc = _fma(acc, w3[:, j], s2[..., j, None])
        return (acc + emb).reshape(n, g * g, C)
    t1 = torch.einsum("cde,iyxpqde->iyxpqc", w1.abs(), m.abs())
    a1 = b1 + torch.einsum("cde,iyxpqde->iyxpqc", w1, m)
    e_a1 = (4 + 2) * U32 * (b1.abs() + t1)
    if loss == "ln_wrong_axis":       # over the four positions of a channel, not over the channels of a position
        x = a1.reshape(n, g, g, 4, c1).transpose(-1, -2)
        s1 = norm_form(0, x, torch.ones(4), None, LN_EPS, act=0, y_f32=True)[0].transpose(-1, -2).reshape(a1.shape)
        s1 = torch.nn.functional.gelu(W["g1"].double() * s1 + W["be1"].double())
        e_s1 = torch.zeros_like(s1)
    else:
        s1, bn1, carry1 = _ln_gelu(a1, W["g1"], W["be1"], loss="no_eps" if loss == "no_eps" else None)
        e_s1 = bn1 + carry1(e_a1)
    a2 = b2 + torch.einsum("kcpq,iyxpqc->iyxk", w2, s1)
    e_a2 = (4 * c1 + 2) * U32 * (b2.abs() + torch.einsum("kcpq,iyxpqc->iyxk", w2.abs(), s1.abs())) + \
        torch.einsum("kcpq,iyxpqc->iyxk", w2.abs(), e_s1)
    s2, bn2, carry2 = _ln_gelu(a2, W["g2"], W["be2"], loss=loss if loss in ("no_eps", "gelu2_missing") else None)
    e_s2 = bn2 + carry2(e_a2)
    dense = b3 + torch.einsum("kj,iyxj->iyxk", w3, s2)
    e_d = (c2 + 2) * U32 * (b3.abs() + torch.einsum("kj,iyxj->iyxk", w3.abs(), s2.abs())) + \
        torch.einsum("kj,iyxj->iyxk", w3.abs(), e_s2)
    if loss == "dense_prompt0":
        assert n >= 2
        dense = dense[:1].expand(n, -1, -1, -1)
    ref = dense if loss == "emb_not_added" else dense + emb
    bound = e_d + U32 * ref.abs()
    return ref.reshape(n, g * g, C), (None if loss else bound.reshape(n, g * g, C))


# (n, g, C, c1, c2, max_wg): the three shapes of the issue; max_wg = 3 on the first makes 13 tiles take a grid-stride tail
EMBED_CASES = [(1, 14, 256, 4, 16, 3), (2, 5, 64, 4, 16, 0), (1, 1, 8, 2, 4, 0)]
EMBED_REFUSED = [dict(c1=9), dict(c2=33), dict(C=6), dict(C=1028)]


def embed_weights(C, c1, c2, gen):
    r = lambda *s: torch.randn(*s, generator=gen)
    # (b1 small: in a flat region of the mask conv 1 leaves its biases alone, and the norm's eps shows against their variance)
    return dict(w1=r(c1, 1, 2, 2) / 2, b1=r(c1) * 0.005, g1=1 + 0.1 * r(c1), be1=r(c1) * 0.05,
                w2=r(c2, c1, 2, 2) / (4 * c1) ** 0.5, b2=r(c2) * 0.05, g2=1 + 0.1 * r(c2), be2=r(c2) * 0.05,
                w3=r(C, c2) / c2 ** 0.5, b3=r(C) * 0.05)


def embed_case(n, g, C, c1, c2, max_wg=0):
    gen = _gen(n, g, C, c1, c2, 43)
    W = embed_weights(C, c1, c2, gen)
    mask = torch.randn(n, 4 * g, 4 * g, generator=gen) * 4
    # a flat region (logits ~ 1e-4: conv 1 leaves little more than its biases, whose variance is ~ 1e-5): the only place
    # where the norm's eps is visible.  At g = 1 that is the whole mask.
    mask[:, : max(4, 2 * g), : max(4, 2 * g)] *= 2.5e-5
    emb = torch.randn(g * g, C, generator=gen) * 0.5
    ref, bound = mask_prompt_embed(mask, emb, W, g)
    losses = [k for k in EMBED_LOSSES if k != "dense_prompt0" or n >= 2]
    muts = {k: mask_prompt_embed(mask, emb, W, g, loss=k)[0] for k in losses}
    return dict(mask=mask, emb=emb, W=W, ref=ref, bound=bound, mutants=muts)


# =====================================================================================================================
# the two f32 attention forms of the prompted decoder (through the existing anyref_op_attention): (B, H, Sq, Sk, hd)
# =====================================================================================================================
ATTN_CASES = [(2, 8, 10, 10, 32), (2, 8, 10, 196, 16), (2, 8, 196, 10, 16)]
