"""Float64 references, derived per-element bounds and mutants for the GEMM / norm / attention launch forms the model
itself uses (tests/test_gpu_gemm_forms.py runs the kernels against them, tests/test_cpu_gemm_forms_ref.py proves on the
CPU that every bound admits an f32 emulation of the kernel and rejects every mutant).  Plain torch on whatever device
the operands are on; nothing here needs a GPU or the HIP library.

Conventions (those of tests/test_gpu_ops.py): the reference is float64 over the operands AS STORED, so a product of two
16-bit values is exact and the legitimate differences are the f32 summation order, the f32 epilogue and the rounding of
the output to its storage type.  A bound is a sum of such terms, each written down where it is added; none is tuned to
what a kernel returns.  A mutant is the same reference with one plausible loss; it must break the bound somewhere.

Storage type ids (include/anyref_hip_ops.h): 0 f32, 1 bf16, 2 f16, 3 bf16 pairs x bf16 weights, 4 f16 pairs x f16 weights.
"""
import math

import torch

U32 = 2.0 ** -24                      # unit roundoff of f32
U16 = {1: 2.0 ** -8, 2: 2.0 ** -11}   # unit roundoff of bf16 / f16: the rounding of a 16-bit output
DROP_K = 8                            # the lost K chunk: one 16-byte load of 16-bit values
_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16, 3: torch.bfloat16, 4: torch.float16}
ACT_NONE, ACT_RELU, ACT_GELU, ACT_QUICK_GELU, ACT_SILU = 0, 1, 2, 3, 4
_ACTS = [lambda z: z, torch.relu, torch.nn.functional.gelu, lambda z: z * torch.sigmoid(1.702 * z),
         torch.nn.functional.silu]
# f32 arithmetic of a fused / stand-alone norm, in units of 2^-24 of |y|: the sum of squares (4 * MAXV <= 8 per thread, 6
# wave steps, <= 16 waves: <= 30 roundings, halved by the square root = 15), the division by N and the + eps (2, halved = 1),
# rsqrtf (1 ulp = 2), the two multiplies and the bias add (3), the mean subtraction of LayerNorm (1), spare 2
NORM_UNITS = 24
PAIR_MUL = 2.0 ** -15                  # a product of two bf16 pairs on three passes (attention_form)


def wdtype(ty):
    return _DT[ty]


def rnd(t, ty):
    """what a kernel sees of a weight / a 16-bit activation after storage rounding"""
    return t.to(_DT[ty]).float()


def terms(a, ty):
    """the 16-bit terms an f32 activation is carried as (t = 3 / 4: hi + lo; t = 1 / 2: the rounded value; t = 0: itself)"""
    if ty in (0, 1, 2):
        return [rnd(a, ty)]
    hi = a.to(_DT[ty]).float()
    lo = (a - hi).to(_DT[ty]).float()
    return [hi, lo]


def eff64(a, ty):
    """float64 value of the stored activation, and the sum of its terms' magnitudes (what the accumulation bound sees)"""
    ts = [x.double() for x in terms(a, ty)]
    return sum(ts), sum(x.abs() for x in ts)


def out_round_bound(y, ty, f32_out=False):
    """rounding of a finished f32 value y to the output's storage type: nothing for f32; one 16-bit rounding for bf16 / f16
    (f16: at least half a subnormal step, 2^-25); for split pairs the residual of hi + lo.  bf16 pairs: with 2^e <= |y| <
    2^(e+1), |y - hi| <= 2^(e-8) lies in a binade below 2^(e-8), whose half step is 2^(e-17): <= 2^-17 |y| (the constant of
    test_gpu_parity16's round trip; 2^-18 is the typical, not the worst case -- the CPU emulation exceeds it).  f16 pairs:
    max(2^-22 |y|, 2^-25), the unit of tests/test_gpu_parity16_f16_ops.pair_bound"""
    if f32_out or ty == 0:
        return torch.zeros_like(y)
    if ty == 1:
        return U16[1] * y.abs()
    if ty == 2:
        return (U16[2] * y.abs()).clamp_min(2.0 ** -25)
    if ty == 3:
        return 2.0 ** -17 * y.abs()
    return torch.maximum(y.abs() * 2.0 ** -22, torch.full_like(y, 2.0 ** -25))


def round_out(y, ty, f32_out=False):
    """the emulation's output store"""
    if f32_out or ty == 0:
        return y.float()
    return sum(terms(y.float(), ty))


def gemm_acc_bound(Aabs, Wabs, K):
    """f32 accumulation of A W^T with K products: one f32 rounding per product, c = K + 32 (+ 32 for the split-K / epilogue
    adds): c * 2^-24 * sum_k |a_k w_k|"""
    return (K + 32) * U32 * (Aabs @ Wabs.transpose(-1, -2))


def ratio(x, ref, bound):
    """worst |x - ref| / bound; a zero bound (an output that must stay exactly as it was) admits no error at all"""
    x, ref, bound = x.double(), ref.double(), bound.double()
    e = (x - ref).abs()
    inf = torch.full_like(e, math.inf)
    r = torch.where(bound > 0, e / bound.clamp_min(1e-300), torch.where(e > 0, inf, torch.zeros_like(e)))
    r = torch.where(torch.isfinite(x), r, inf)
    return r.max().item()


def check_bound(got, ref, bound, mutants, what):
    """per-element |got - ref| <= bound; and every mutant reference (one plausible loss each) must break the same bound on
    at least one element -- a bound too loose to see that loss fails the test by itself.  mutants: a tensor or {name: tensor}"""
    ref = ref.double()
    got = got.to(ref.device).double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    r = ratio(got, ref, bound)
    assert r <= 1.0, f"{what}: worst error / bound = {r:.3f}"
    if not isinstance(mutants, dict):
        mutants = {"mutant": mutants}
    ms = {}
    for name, m in mutants.items():
        ms[name] = ratio(m.to(ref.device), ref, bound)
        assert ms[name] > 1.0, f"{what}: the mutant '{name}' stays inside the bound (worst ratio {ms[name]:.3f})"
    print(f"{what}: worst error / bound {r:.3g}; mutants " + ", ".join(f"{k} {v:.3g}" for k, v in ms.items()))
    return r


# ---------------------------------------------------------------------------------------------------------------------
# GEMM forms.  Logical operands (the test lays them out with whatever strides the form has):
#   A [Z, Ma, K] f32 (Z = batch, or 1), W [Zw, N, K] (Zw = Z or 1: shared), bias [Zb, N], resid [Zr, Mr, N]
#   a_row_map [M]: row of A for logical row m; row_map [M]: destination row, < 0 dropped; C0 [Z, rows, N]: what C held
# One function computes the float64 reference and the bound of everything the launch writes; `loss` names the ONE line a
# mutant changes.  emulate=True computes the same thing the way a kernel does (f32, per K slice, slabs in order).
# ---------------------------------------------------------------------------------------------------------------------
LOSSES = ("drop_k", "norm_before_resid", "no_eps", "ln_keeps_mean", "swap_gate_up", "not_interleaved", "slab_missing",
          "slab_swapped", "z_on_shared_w", "alpha_ignored", "block_shift", "resid_per_batch")


def _act64(z, act):
    return _ACTS[act](z)


def gemm_form(ty, A, W, *, bias=None, resid=None, alpha=1.0, act=ACT_NONE, c_f32=True, swiglu=False, slabs=0,
              norm=None, row_map=None, a_row_map=None, C0=None, loss=None, emulate=False, splits=1, block_rows=0,
              k_real=0):
    """returns {"C": (ref, bound), "norm": (ref, bound), "slabs": (ref, bound)} (the entries the form writes); with
    emulate=True the tensors are the f32 emulation's outputs instead of (ref, bound) pairs.
    norm: {"gain", "bias" (None: RMSNorm), "eps"}; block_rows: rows per launch of a capped 256-row-tile launch (for the
    block_shift loss only); k_real: the K columns that carry weights when the rest is zero padding (drop_k loses the last
    chunk of those)."""
    dev = A.device
    Z, _, K = A.shape
    N = W.shape[1]
    Wr = rnd(W, ty)
    if loss == "drop_k":
        Wr = Wr.clone()
        if slabs > 1:        # the last chunk of every K slice
            for z in range(slabs):
                Wr[..., (z + 1) * K // slabs - DROP_K:(z + 1) * K // slabs] = 0
        else:
            Wr[..., (k_real or K) - DROP_K:(k_real or K)] = 0
    if loss == "z_on_shared_w":      # W + z * (one row) instead of W: batch z reads the table shifted by z rows
        assert W.shape[0] == 1 and Z > 1
        Wr = torch.stack([torch.roll(Wr[0], -z, 0) for z in range(Z)])
    Asrc = A
    if a_row_map is not None:
        Asrc = A[:, a_row_map.long()]
    M = Asrc.shape[1]
    if loss == "block_shift":        # the second row block reads A one 256-row tile further on
        assert block_rows > 0 and M > block_rows + 256
        Asrc = Asrc.clone()
        Asrc[:, block_rows:M - 256] = Asrc[:, block_rows + 256:].clone()
    if loss == "alpha_ignored":
        alpha = 1.0
    ts = terms(Asrc, ty)
    nk = max(1, slabs if slabs > 1 else splits)
    ks = [(z * K // nk, (z + 1) * K // nk) for z in range(nk)]

    if emulate:
        # f32 matmul per K slice and term, slices summed in slab order
        parts = [sum(t[..., a:b] @ Wr[..., a:b].transpose(-1, -2) for t in ts) for a, b in ks]
        if slabs > 1:
            return {"slabs": torch.stack([p[0] for p in parts])}
        z = parts[0]
        for p in parts[1:]:
            z = z + p
        z = z * torch.tensor(alpha, dtype=torch.float32)
        f = lambda x: x                                          # noqa: E731
        absA = absW = None
    else:
        f = lambda x: x.double()                                 # noqa: E731
        A64 = sum(f(t) for t in ts)
        absA = sum(f(t).abs() for t in ts)
        W64, absW = f(Wr), f(Wr).abs()
        if slabs > 1:
            order = list(range(slabs))
            if loss == "slab_swapped":
                order = order[::-1]
            ref = torch.stack([(A64[..., a:b] @ W64[..., a:b].transpose(-1, -2))[0] for a, b in (ks[i] for i in order)])
            if loss == "slab_missing":
                ref[-1] = 0
            bnd = torch.stack([gemm_acc_bound(absA[..., a:b], absW[..., a:b], (b - a) * len(ts))[0] for a, b in ks])
            return {"slabs": (ref, bnd)}
        z = alpha * (A64 @ W64.transpose(-1, -2))
        ez = abs(alpha) * gemm_acc_bound(absA, absW, K * len(ts)) + U32 * z.abs()      # + the multiply by alpha

    out = {}
    if swiglu:
        z1, z2 = z[..., 0::2], z[..., 1::2]
        if loss == "swap_gate_up":
            z1, z2 = z2, z1
        if loss == "not_interleaved":
            z1, z2 = z[..., :N // 2], z[..., N // 2:]
        sz = torch.nn.functional.silu(z1)
        c = sz * z2
        if emulate:
            return {"C": round_out(c, ty, c_f32)}
        e1, e2 = ez[..., 0::2], ez[..., 1::2]
        # product rule (the GEMV test's): silu' <= 1.1; the f32 silu and product within 8 units of 2^-24
        b = 1.1 * e1 * (z2.abs() + e2) + sz.abs() * e2 + 8 * U32 * c.abs()
        b = b + out_round_bound(c.abs() + b, ty, c_f32)
        return {"C": (c, b)}

    if bias is not None:
        z = z + f(bias)[:, None, :]
    c = _act64(z, act)
    if not emulate:
        # z's error goes through the activation (|act'| <= 1.2 for all five), the f32 activation itself is within 16 units
        # of 2^-24 of its value (test_gpu_ops.test_gemm); nothing of either without an activation
        e = (1.2 * (ez + U32 * z.abs()) + 16 * U32 * c.abs()) if act != ACT_NONE else ez + U32 * z.abs()
    pre = c
    if resid is not None:
        r = f(resid)
        if loss == "resid_per_batch":      # the shared residual read at batch stride M * N: batch z gets rows shifted by z
            r = torch.stack([torch.roll(r[0], -z_, 0) for z_ in range(Z)])
        c = c + r
        if not emulate:
            e = e + U32 * c.abs()
    # ---- C ----
    if emulate:
        cst = round_out(c, ty, c_f32)
    else:
        bC = e + out_round_bound(c.abs() + e, ty, c_f32)
    if row_map is not None or C0 is not None:
        tgt = row_map.long() if row_map is not None else torch.arange(M, device=dev)
        sel = tgt >= 0
        full = (C0.float() if emulate else C0.double()).clone()
        full[:, tgt[sel]] = (cst if emulate else c)[:, sel]
        if emulate:
            cst = full
        else:
            fb = torch.zeros_like(full)
            fb[:, tgt[sel]] = bC[:, sel]
            c_full, bC = full, fb
    else:
        c_full = c
    out["C"] = cst if emulate else (c_full, bC)
    # ---- the norm fused into the split-K reduction (on the f32 row, before C is rounded) ----
    if norm is not None:
        g, nb, eps = f(norm["gain"]), norm["bias"], norm["eps"]
        v = pre if loss == "norm_before_resid" else c
        if loss == "no_eps":
            eps = 0.0
        if nb is not None:      # LayerNorm
            mu = v.mean(-1, keepdim=True)
            d = v if loss == "ln_keeps_mean" else v - mu
        else:
            d = v
        rs = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
        y = g * d * rs
        if nb is not None:
            y = y + f(nb)
        if emulate:
            out["norm"] = round_out(y, ty, False)
        else:
            ed = e
            if nb is not None:
                # d_n = c_n - mean c: the mean moves by at most mean e, its own f32 sum (<= 32 roundings of partial sums
                # of |c|) and the subtraction's rounding
                ed = e + e.mean(-1, keepdim=True) + 32 * U32 * v.abs().mean(-1, keepdim=True) + U32 * d.abs()
            # dy_n = g_n (dd_n r + d_n dr), dr = -r^3 mean_j(d_j dd_j)
            by = g.abs() * rs * (ed + d.abs() * rs * rs * (d.abs() * ed).mean(-1, keepdim=True))
            by = by + NORM_UNITS * U32 * ((g * d * rs).abs() + y.abs())
            by = by + out_round_bound(y.abs() + by, ty, False)
            out["norm"] = (y, by)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Norm forms
# ---------------------------------------------------------------------------------------------------------------------
def norm_form(ty, x, gain, bias, eps, *, rms=False, act=ACT_NONE, y_f32=False, row_map=None, Y0=None, loss=None,
              emulate=False):
    """y[row_map[m]] = act(norm(x[m]) * gain + bias), rows with row_map < 0 dropped (Y0 [rows, D] kept there, zero bound).
    x is f32 and exact; the bound is the f32 arithmetic alone: the statistics (NORM_UNITS), the activation (16 units,
    slope <= 1.2) and the output rounding.  losses: row_map_ignored, act_dropped, no_eps."""
    f = (lambda t: t.float()) if emulate else (lambda t: t.double())
    x, g = f(x), f(gain)
    if loss == "no_eps":
        eps = 0.0
    d = x if rms else x - x.mean(-1, keepdim=True)
    rs = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    z = g * d * rs
    if bias is not None:
        z = z + f(bias)
    y = z if loss == "act_dropped" else _act64(z, act)
    if not emulate:
        # (mean subtraction: the f32 mean is off by <= 32 * 2^-24 mean |x|, which moves every d_n by that much)
        ed = torch.zeros_like(x) if rms else 32 * U32 * x.abs().mean(-1, keepdim=True) + U32 * d.abs()
        bz = g.abs() * rs * (ed + d.abs() * rs * rs * (d.abs() * ed).mean(-1, keepdim=True))
        bz = bz + NORM_UNITS * U32 * ((g * d * rs).abs() + z.abs())
        b = bz if act == ACT_NONE else 1.2 * bz + 16 * U32 * y.abs()
        b = b + out_round_bound(y.abs() + b, ty, y_f32)
    else:
        y = round_out(y, ty, y_f32)
    if row_map is not None or Y0 is not None:
        M = x.shape[0]
        tgt = row_map.long() if (row_map is not None and loss != "row_map_ignored") else torch.arange(M, device=x.device)
        sel = tgt >= 0
        full = f(Y0).clone()
        full[tgt[sel]] = y[sel]
        if emulate:
            return full
        fb = torch.zeros_like(full)
        fb[tgt[sel]] = b[sel]
        return full, fb
    return y if emulate else (y, b)


def fill_form(ty, dst0, rows, bias, N, *, gain=None, loss=None):
    """the side job: dst[rows[i], 0:N) = T(bias), everything else as it was.  Exact: the bound is the output rounding of
    the bias alone and zero off the filled rows.  losses: gain_scaled (gain * bias written), rows_unmapped (row i, not rows[i])"""
    ref = dst0.double().clone()
    bnd = torch.zeros_like(ref)
    b = bias.double()[:N]
    if loss == "gain_scaled":
        b = b * gain.double()[:N]
    idx = rows.long() if loss != "rows_unmapped" else torch.arange(rows.numel(), device=rows.device)
    ref[idx, :N] = b
    bnd[rows.long(), :N] = out_round_bound(bias.double()[:N], ty if ty in (1, 2) else 0)
    return ref, bnd


# ---------------------------------------------------------------------------------------------------------------------
# Attention forms: q / k / v are LOGICAL [B, S, H, hd] tensors (the test lays them into fused buffers / caches).
# ---------------------------------------------------------------------------------------------------------------------
def attention_form(ty, q, k, v, scale, *, causal=False, kv_len=None, q_len=None, q_pos0=None, rel_h=None, rel_w=None, kw=0,
                   rel_abs=None, rel_pairs=False, O0=None, loss=None, k_wrong=None, tile=64):
    """float64 attention over the stored q / k / v with the per-element bound of tests/test_gpu_ops.attention_bound64 (the
    same terms: scores (hd + 16) 2^-24 sum |q k| scale, exp within 2^-21 (1 + |s - M|), P rounded to T, P V with one
    rounding per 4 keys, the output rounding; t = 0: no 16-bit rounding, P V one f32 rounding per key).  Rows >= q_len[b]
    keep O0 with a zero bound.
    q_pos0[b]: position of query row 0 (causal over a cache: key j visible iff j <= q_pos0[b] + i); rel_pairs: the bias is
    computed by the t = 3 kernel itself from the tables (pair products: PAIR_MUL of rel_abs more on the scores).
    losses: drop_tile (the last `tile` keys of every row), q_pos0_ignored, k_wrong (keys read from k_wrong: the q columns of the fused
    buffer), q_len_ignored (every row written)."""
    q, k, v = (x.double() for x in (q, k, v))
    if loss == "k_wrong":
        k = k_wrong.double()
    B, Sq, H, hd = q.shape
    Sk = k.shape[1]
    dev = q.device
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    es = (hd + 16) * U32 * torch.einsum("bqhd,bkhd->bhqk", q.abs(), k.abs()) * scale
    if rel_h is not None:
        kh = rel_h.shape[-1]
        s = (s.view(B, H, Sq, kh, kw) + rel_h.double()[..., :, None] + rel_w.double()[..., None, :]).view(B, H, Sq, Sk)
        if rel_abs is not None:
            rah, raw = (x.double() for x in rel_abs)
            es = es + ((hd + 16) * U32 * (rah[..., :, None] + raw[..., None, :])).reshape(B, H, Sq, Sk)
    mask = torch.zeros(B, 1, Sq, Sk, dtype=torch.bool, device=dev)
    n = [Sk] * B
    if kv_len is not None:
        for b in range(B):
            mask[b, :, :, int(kv_len[b]):] = True
            n[b] = int(kv_len[b])
    if causal:
        tri = torch.ones(Sq, Sk, dtype=torch.bool, device=dev)
        p0 = [0] * B if (q_pos0 is None or loss == "q_pos0_ignored") else [int(x) for x in q_pos0]
        mask = mask | torch.stack([tri.triu(1 + p0[b]) for b in range(B)])[:, None]
    if loss == "drop_tile":
        for b in range(B):
            mask[b, :, :, max(1, n[b] - tile): n[b]] = True
    dead = mask.expand(B, 1, Sq, Sk).all(-1, keepdim=True)
    mask = mask & ~dead
    s = s.masked_fill(mask, float("-inf"))
    pr = torch.softmax(s, -1)
    o = torch.einsum("bhqk,bkhd->bqhd", pr, v)
    pv = torch.einsum("bhqk,bkhd->bqhd", pr, v.abs())
    m = s.max(-1, keepdim=True).values
    delta = (es + es.masked_fill(mask, 0).amax(-1, keepdim=True) + 2.0 ** -21 * (1 + (s - m).abs())).masked_fill(mask, 0)
    dt = torch.einsum("bhqk,bkhd->bqhd", pr * delta, v.abs()) + (pr * delta).sum(-1).permute(0, 2, 1)[..., None] * o.abs()
    if ty == 0:
        # t = 0: f32 operands on the f32 MFMA, P and the output stay f32 -- the same terms without the two 16-bit roundings;
        # P V adds one key per f32 MFMA step, so one f32 rounding per key: the figure of
        # tests/test_gpu_decode_ops.decode_bound for the f32 fallback (proved by tests/test_cpu_attn_peaked_ref.py)
        bound = dt + 2 * (Sk + 64) * U32 * pv
    elif ty in (1, 2):
        u = U16[ty]
        bound = dt + u * (pv + 2 * o.abs()) + 2 * (Sk / 4 + 64) * U32 * pv
    else:
        # t = 3: f32 operands multiplied as bf16 PAIRS in three passes (hi hi, hi lo, lo hi).  Each operand is hi + lo + r with
        # |lo| <= 2^-8 |a| and |r| <= 2^-17 |a| (out_round_bound): a product loses lo lo (<= 2^-16 |a b|) and the two
        # residuals (2 x 2^-17 |a b|) = PAIR_MUL = 2^-15 of sum |a b|; three times the f32 roundings of one pass
        assert ty == 3, "attention_form: t = 0 / 1 / 2 / 3"
        dq = (PAIR_MUL + 2 * (hd + 16) * U32) * torch.einsum("bqhd,bkhd->bhqk", q.abs(), k.abs()) * scale
        if rel_pairs:
            assert rel_abs is not None, "rel_pairs needs rel_abs (sum |q| |R| of the bias dot products)"
            dq = dq + (PAIR_MUL * (rah[..., :, None] + raw[..., None, :])).reshape(B, H, Sq, Sk)
        d3 = (dq + dq.masked_fill(mask, 0).amax(-1, keepdim=True)).masked_fill(mask, 0)
        dt = dt + torch.einsum("bhqk,bkhd->bqhd", pr * d3, v.abs()) + (pr * d3).sum(-1).permute(0, 2, 1)[..., None] * o.abs()
        bound = dt + PAIR_MUL * (pv + 2 * o.abs()) + 6 * (Sk / 4 + 64) * U32 * pv
        bound = bound + out_round_bound(o.abs() + bound, ty)
    if q_len is not None and loss != "q_len_ignored":
        keep = torch.zeros(B, Sq, dtype=torch.bool, device=dev)
        for b in range(B):
            keep[b, int(q_len[b]):] = True
        o = torch.where(keep[..., None, None], O0.double(), o)
        bound = torch.where(keep[..., None, None], torch.zeros_like(bound), bound)
    return o, bound


def attention_emulate(ty, q, k, v, scale, *, causal=False, kv_len=None, q_len=None, q_pos0=None, rel_h=None, rel_w=None,
                      kw=0, O0=None, tile=64):
    """the kernel's arithmetic in f32 torch: f32 scores from the stored operands, online softmax over key tiles of `tile`
    with P rounded to T before P V, the output rounded to T; rows >= q_len not written.
    The order is the textbook one (natural exp, the maximum moved by every tile that raises it); the kernels' own lazy rule
    in log2 units -- which matters once scores are peaked -- is tests/attn_peaked_ref.attention_kernel_order"""
    def mul3(eq, a, b):      # t = 3: three passes over the pair terms; 16-bit types: the one product
        if ty != 3:
            return torch.einsum(eq, rnd(a, ty), rnd(b, ty))
        (ah, al), (bh, bl) = terms(a, 3), terms(b, 3)
        return torch.einsum(eq, ah, bh) + torch.einsum(eq, ah, bl) + torch.einsum(eq, al, bh)
    q, k, v = (x.float() for x in (q, k, v))
    B, Sq, H, hd = q.shape
    Sk = k.shape[1]
    s = mul3("bqhd,bkhd->bhqk", q, k) * torch.tensor(scale, dtype=torch.float32)
    if rel_h is not None:
        kh = rel_h.shape[-1]
        s = (s.view(B, H, Sq, kh, kw) + rel_h.float()[..., :, None] + rel_w.float()[..., None, :]).view(B, H, Sq, Sk)
    mask = torch.zeros(B, 1, Sq, Sk, dtype=torch.bool)
    if kv_len is not None:
        for b in range(B):
            mask[b, :, :, int(kv_len[b]):] = True
    if causal:
        tri = torch.ones(Sq, Sk, dtype=torch.bool)
        mask = mask | torch.stack([tri.triu(1 + (int(q_pos0[b]) if q_pos0 is not None else 0)) for b in range(B)])[:, None]
    s = s.masked_fill(mask, float("-inf"))
    m = torch.full((B, H, Sq, 1), -1e30)
    l = torch.zeros(B, H, Sq, 1)
    acc = torch.zeros(B, H, Sq, hd)
    for j in range(0, Sk, tile):
        st = s[..., j:j + tile]
        mn = torch.maximum(m, st.amax(-1, keepdim=True))
        p = torch.exp(st - mn)
        c = torch.exp(m - mn)
        pt = rnd(p, ty) if ty != 3 else p
        l = l * c + pt.sum(-1, keepdim=True)
        acc = acc * c + mul3("bhqk,bkhd->bhqd", pt, v[:, j:j + tile])
        m = mn
    o = round_out((acc / l).permute(0, 2, 1, 3), ty)
    if q_len is not None:
        for b in range(B):
            o[b, int(q_len[b]):] = O0[b, int(q_len[b]):].float()
    return o


# ---------------------------------------------------------------------------------------------------------------------
# The raw slabs chained into the RoPE + cache kernel: x = T(slab0 + slab1) (t = 0: the f32 sum), q / k rotated, v stored
# ---------------------------------------------------------------------------------------------------------------------
def rope_chain_form(ty, x, ex, cs, sn):
    """x, ex: float64 [S, 3, H, hd] qkv projection and its accumulation bound (the sum of the two slabs' bounds); cs, sn
    [S, hd / 2] the table rows.  Returns {"q", "k", "v"}: (ref, bound) of the rows the kernel writes.  The sum is rounded to T
    once (ex grows by that rounding), the rotation a = x1 c - x2 s, b = x2 c + x1 s is f32 (2 roundings per term, the bound
    of tests/test_gpu_decode_ops.rotate64) and the result rounded to T once more."""
    ex = ex + U32 * x.abs()                                  # the f32 add of the two slabs
    ex = ex + out_round_bound(x.abs() + ex, ty)
    half = x.shape[-1] // 2
    cs, sn = cs.double()[:, None, :], sn.double()[:, None, :]

    def rot(xx, ee):
        x1, x2, e1, e2 = xx[..., :half], xx[..., half:], ee[..., :half], ee[..., half:]
        a, b = x1 * cs - x2 * sn, x2 * cs + x1 * sn
        ea = e1 * cs.abs() + e2 * sn.abs() + 2 * U32 * ((x1 * cs).abs() + (x2 * sn).abs())
        eb = e2 * cs.abs() + e1 * sn.abs() + 2 * U32 * ((x2 * cs).abs() + (x1 * sn).abs())
        r, e = torch.cat([a, b], -1), torch.cat([ea, eb], -1)
        return r, e + out_round_bound(r.abs() + e, ty)
    return {"q": rot(x[:, 0], ex[:, 0]), "k": rot(x[:, 1], ex[:, 1]), "v": (x[:, 2], ex[:, 2])}


def rope_chain_emulate(ty, slab0, slab1, cs, sn):
    """f32: the slab sum rounded to T, the f32 rotation, the result rounded to T"""
    x = round_out(slab0.float() + slab1.float(), ty)
    half = x.shape[-1] // 2
    cs, sn = cs.float()[:, None, :], sn.float()[:, None, :]

    def rot(xx):
        x1, x2 = xx[..., :half], xx[..., half:]
        return round_out(torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1), ty)
    return {"q": rot(x[:, 0]), "k": rot(x[:, 1]), "v": x[:, 2]}


# ---------------------------------------------------------------------------------------------------------------------
# operands shared by the CPU proof and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def gemm_operands(M, N, K, seed, *, Z=1, Zw=1, w_scale=0.05, small_rows=False, row_offset=False, with_bias=False):
    """A [Z, M, K], W [Zw, N, K], bias [Z, N], resid [Z, M, N], gain, nbias [N].  small_rows: every 5th row of A and resid
    is scaled so that the finished row has magnitude ~ 1e-3 = sqrt(eps = 1e-6) (a norm without eps is then off by tens
    of per cent there; with_bias: the residual of those rows also cancels the GEMM's bias); row_offset: resid carries a per-row mean (LayerNorm that keeps the mean is then far off)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(Z, M, K, generator=g)
    W = torch.randn(Zw, N, K, generator=g) * w_scale
    bias = torch.randn(Z, N, generator=g) * 0.5
    resid = torch.randn(Z, M, N, generator=g)
    if row_offset:
        resid = resid + 2.0 * torch.randn(Z, M, 1, generator=g)
    if small_rows:
        A[:, ::5] *= 1e-3 / (w_scale * math.sqrt(K))
        resid[:, ::5] *= 1e-3
        if with_bias:
            resid[:, ::5] -= bias[:, None, :]
    gain = 1 + 0.2 * torch.randn(N, generator=g)
    nbias = 0.3 * torch.randn(N, generator=g)
    return A, W, bias, resid, gain, nbias
