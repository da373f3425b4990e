"""Kernel-level tests of the decode-step kernels (include/anyref_hip_ops.h): the RoPE table, the fused decode attention
(RoPE + KV append + one-query attention) and its fallback, the prefill RoPE + KV append family, the greedy argmax (plain and
with the next step's bookkeeping) and the f32 normalised rows of the lm_head GEMV.

Every reference is float64 torch over exactly the values the kernel stores (the T-rounded rotated q / k, the T cache rows);
every bound is written next to the arithmetic it follows, and the attention bound is checked to be tight enough to see a
dropped key (the mutant self-check)."""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24                                   # unit roundoff of f32
_DT = {0: torch.float32, 1: torch.bfloat16}        # t of the entries: 0 = f32, 1 = bf16 storage
_P_BITS = {0: 24, 1: 8}                            # significand bits (implicit bit included)
THETA = 10000.0


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


_KEEP = []


def P(t):
    if t is None:
        return None
    _KEEP.append(t)
    return C.c_void_p(t.data_ptr())


def check(lib, rc):
    assert rc == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()
    _KEEP.clear()


def ulp(x, t):
    """one unit in the last place of type t at |x| (float64; the smallest normal for 0)"""
    _, e = torch.frexp(x.abs().clamp_min(1e-30))
    return torch.ldexp(torch.ones_like(x), (e - _P_BITS[t]).to(torch.int32))


def rope_table(lib, S, hd):
    tab = torch.empty(S, 2, hd // 2)
    check(lib, lib.anyref_op_rope_table(S, hd, THETA, C.c_void_p(tab.data_ptr())))
    return tab


def rotate64(x1, x2, cs, sn):
    """float64 rotation of the f32 operands (x1, x2 the two halves) and the f32 rounding allowance of the kernel's
    x1 * cs - x2 * sn: at most two f32 roundings of terms of size |x1 cs| + |x2 sn| (fma or not)"""
    x1, x2, cs, sn = (v.double() for v in (x1, x2, cs, sn))
    a, b = x1 * cs - x2 * sn, x2 * cs + x1 * sn
    ea = 2 * U32 * (x1.abs() * cs.abs() + x2.abs() * sn.abs())
    eb = 2 * U32 * (x2.abs() * cs.abs() + x1.abs() * sn.abs())
    return torch.cat([a, b], -1), torch.cat([ea, eb], -1)


def assert_rounded(got, exact, f32err, t, what):
    """got (stored in T) within one unit in the last place of T of the float64 value, plus the f32 rounding of the
    rotation itself (that term is what makes the f32 check meaningful under cancellation)"""
    got = got.double()
    err = (got - exact).abs()
    bound = ulp(exact, t) + f32err
    r = (err / bound).max().item()
    assert r <= 1.0, f"{what}: worst error / (1 ulp + f32 rounding) = {r:.3f}"
    return r


# ----------------------------------------------------------------------------------------------------------------------
# RoPE table
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,S", [(64, 4096), (128, 4096), (128, 330)])
def test_rope_table(lib, hd, S):
    """the table the model uploads (rope_table in ops.hip) against HF's fp32 formula (the oracle) and float64.
    Bound per entry |pos * inv| * c * 2^-23 + 2^-23, c = 8: the f32 exponent 2d/hd is rounded (relative 2^-24, which
    ln(theta) = 9.2 turns into 9.2 * 2^-24 of theta^e), powf and the division add ~2 units, pos * inv one more -- so the
    angle is off by at most ~13 * 2^-24 = 6.5 * 2^-23 of itself; cos / sin add ~1 unit of 2^-24 around |value| <= 1."""
    from oracle.anyref_oracle import _rope_cos_sin
    tab = rope_table(lib, S, hd).double()
    cos_k, sin_k = tab[:, 0], tab[:, 1]
    pos = torch.arange(S, dtype=torch.float64)
    inv = THETA ** (-torch.arange(0, hd, 2, dtype=torch.float64) / hd)
    ang = pos[:, None] * inv[None]
    bound = ang.abs() * 8 * 2.0 ** -23 + 2.0 ** -23
    for name, got, ref in (("cos", cos_k, ang.cos()), ("sin", sin_k, ang.sin())):
        r = ((got - ref).abs() / bound).max().item()
        assert r <= 1.0, f"{name} vs float64: worst error / bound = {r:.3f}"
    cfg = SimpleNamespace(llm=SimpleNamespace(head_dim=hd, rope_theta=THETA))
    hc, hs = _rope_cos_sin(cfg, torch.arange(S))
    for name, got, ref in (("cos", cos_k, hc[:, : hd // 2]), ("sin", sin_k, hs[:, : hd // 2])):
        r = ((got - ref.double()).abs() / bound).max().item()
        assert r <= 1.0, f"{name} vs HF fp32: worst error / bound = {r:.3f}"
    # the mutant of an off-by-one position breaks the bound
    assert ((tab[1:, 0] - ang[:-1].cos()).abs() / bound[1:]).max() > 1


# ----------------------------------------------------------------------------------------------------------------------
# Decode attention (fused kernel and its fallback)
# ----------------------------------------------------------------------------------------------------------------------
def _kpi(t, hd):
    vec = 16 // (4 if t == 0 else 2)         # elements per 16-byte load
    kpi = 512 // (hd // vec)                 # keys per sweep of the 512-thread workgroup
    un = 6 if t == 0 else 4                  # sweeps per batch (decode_attn.h)
    return kpi, kpi * un


def _decode_positions(t, hd, maxS):
    kpi, bs = _kpi(t, hd)
    ps = [0, 1, kpi - 1, kpi, bs - 1, bs, bs + 1] + list(range(320, 330)) + [maxS - 1]
    return sorted({p for p in ps if p < maxS})


def decode_reference(q, kc, vc, pos, H, hd, scale, drop=0):
    """float64 attention of the stored q (q_keep row) over the stored keys 0..p (key p the row just written), per b;
    drop > 0: the last `drop` of them left out (the mutants).
    Returns out [B, H, hd], P|v| [B, H, hd], the per-key error weight sum_j P_j * delta_j * (|v_j| + |o|)."""
    outs, pvs, dts = [], [], []
    for b, p in enumerate(pos):
        n = max(0, p + 1 - drop)
        qb = q[b].double()                                    # [H, hd]
        kb = kc[b, :n].double().permute(1, 0, 2)              # [H, n, hd]
        vb = vc[b, :n].double().permute(1, 0, 2)
        if n == 0:
            outs.append(torch.zeros_like(qb)); pvs.append(torch.zeros_like(qb)); dts.append(torch.zeros_like(qb))
            continue
        s = torch.einsum("hd,hnd->hn", qb, kb) * scale
        sabs = torch.einsum("hd,hnd->hn", qb.abs(), kb.abs()) * scale
        pr = torch.softmax(s, -1)
        o = torch.einsum("hn,hnd->hd", pr, vb)
        pv = torch.einsum("hn,hnd->hd", pr, vb.abs())
        # relative error of each weight exp(s_j - M): the f32 score (an fma chain of <= 8 products, <= 5 shuffle adds,
        # and the pre-scaled q: 16 * 2^-24 of sum |q k| scale, for key j and for the max), the f32 s_j - M, the exp itself
        # (__expf / expf: within 2^-21 (1 + |s_j - M|)) and one rescale factor of the same size per key batch
        nb = max(1, math.ceil(n / 96))
        es = 16 * U32 * sabs
        delta = es + es.max(-1, keepdim=True).values + 2.0 ** -21 * (1 + (s - s.max(-1, keepdim=True).values).abs()) * (1 + nb)
        dt = torch.einsum("hn,hnd->hd", pr * delta, vb.abs()) + (pr * delta).sum(-1, keepdim=True) * o.abs()
        outs.append(o); pvs.append(pv); dts.append(dt)
    return torch.stack(outs), torch.stack(pvs), torch.stack(dts)


def decode_bound(pv, dt, o, pos, t, hd, fallback):
    """per-element bound of the kernel's f32 result.  Fused kernel: P and O stay f32; every lane group sums its
    ceil(n / KPI) keys in one fma chain, the KPI groups are merged by one more chain of KPI terms, l likewise, then o / l:
    c = ceil(n / KPI) + KPI + 4 roundings of sum P|v| for O and the same for l.  Fallback (generic attention, Sq = 1):
    the keys stream through one workgroup tile after tile, P V accumulates in MFMA order -- k = 4 keys per f32 MFMA,
    16 per bf16 one; without knowing how the MFMA adds inside, one rounding per key (f32) / per 4 keys (bf16) of
    sum P|v|, + 64 for the merges -- and in bf16 P is rounded to bf16 before P V: + 2^-8 sum P|v|."""
    kpi, _ = _kpi(t, hd)
    n = torch.tensor([p + 1 for p in pos], dtype=torch.float64, device=pv.device)[:, None, None]
    c = (n / (4 if t == 1 else 1) + 64) if fallback else (torch.ceil(n / kpi) + kpi + 4)
    bound = 2 * c * U32 * pv + dt + 2 * U32 * o.abs()
    if fallback and t == 1:
        bound = bound + 2.0 ** -8 * pv
    return bound


def _rand_cache(B, maxS, H, hd, t, g):
    return (torch.randn(B, maxS, H, hd, device="cuda", generator=g) * 0.5).to(_DT[t])


@pytest.mark.parametrize("t,hd,H", [(0, 128, 32), (1, 128, 32), (0, 64, 8), (1, 64, 8), (1, 32, 8)])
@pytest.mark.parametrize("maxS", [512, 4096])
def test_decode_attn(lib, t, hd, H, maxS):
    """decode_attn_kernel at ragged positions: p = 0, 1, KPI - 1, KPI, the key batch -1 / 0 / +1, 320..329 (the C2 decode
    context) and maxS - 1 in launches of <= 12 sequences; the same inputs again through the fallback.  Every cache row is
    random (rows > p included: a kernel reading past the key count is seen), row p must be the float64 rotation within
    1 ulp of T, every other row of kc / vc / q_keep bitwise unchanged."""
    g = torch.Generator(device="cuda").manual_seed(hd * 7 + H + maxS + t)
    tab = rope_table(lib, maxS, hd)
    tab_d = tab.cuda()
    scale = hd ** -0.5
    pos_all = _decode_positions(t, hd, maxS)
    worst = {0: 0.0, 1: 0.0}
    for i0 in range(0, len(pos_all), 12):
        pos = pos_all[i0: i0 + 12]
        B = len(pos)
        # a ragged order (the longest sequence is not always the last one)
        pos = pos[::2] + pos[1::2]
        qkv = torch.randn(B, 3 * H * hd, device="cuda", generator=g)
        kc0, vc0, qk0 = (_rand_cache(B, maxS, H, hd, t, g) for _ in range(3))
        pos_d = torch.tensor(pos, dtype=torch.int32, device="cuda")
        for fb in (0, 1):
            kc, vc, qk = kc0.clone(), vc0.clone(), qk0.clone()
            out = torch.full((B, H * hd), float("nan"), device="cuda")
            check(lib, lib.anyref_op_decode_attn(t, None, P(qkv), B, H, hd, P(pos_d), P(tab_d), P(kc), P(vc), maxS, scale,
                                                 P(out), P(qk), fb))
            bi = torch.arange(B, device="cuda")
            pd = pos_d.long()
            # rows other than p: bitwise unchanged
            for name, new, old in (("kc", kc, kc0), ("vc", vc, vc0), ("q_keep", qk, qk0)):
                keep = torch.ones(B, maxS, dtype=torch.bool, device="cuda")
                keep[bi, pd] = False
                assert torch.equal(new[keep], old[keep]), f"{name}: a row other than the appended one changed"
            # row p: the float64 rotation of this step's q / k, v rounded to T
            x = qkv.view(B, 3, H, hd)
            cs, sn = tab_d[pd, 0][:, None, :], tab_d[pd, 1][:, None, :]
            half = hd // 2
            for name, j, buf in (("q_keep", 0, qk), ("kc", 1, kc)):
                ref, e32 = rotate64(x[:, j, :, :half], x[:, j, :, half:], cs, sn)
                assert_rounded(buf[bi, pd], ref, e32, t, f"{name} row p (fallback={fb})")
            assert torch.equal(vc[bi, pd], x[:, 2].to(_DT[t])), "vc row p is not v rounded to T"
            # the output against float64 attention over the stored values
            q = qk[bi, pd].float()
            o, pv, dt = decode_reference(q, kc, vc, pos, H, hd, scale)
            bound = decode_bound(pv, dt, o, pos, t, hd, fb)
            err = (out.view(B, H, hd).double() - o).abs()
            assert torch.isfinite(out).all()
            r = (err / bound).max().item()
            assert r <= 1.0, f"decode attention (fallback={fb}): worst error / bound = {r:.3f}"
            worst[fb] = max(worst[fb], r)
            # mutant: the appended key left out must break the bound
            om, _, _ = decode_reference(q, kc, vc, pos, H, hd, scale, drop=1)
            keep_b = torch.tensor([p > 0 for p in pos], device="cuda")
            assert ((om - o).abs() / bound)[keep_b].max() > 1, "bound too loose to see a dropped appended key"
    print(f"decode_attn t={t} hd={hd} maxS={maxS}: worst error / bound fused {worst[0]:.3g}, fallback {worst[1]:.3g}")


@pytest.mark.parametrize("t", [0, 1])
def test_decode_attn_long_cache_takes_the_fallback(lib, t):
    """maxS > 12000: launch_decode_attn refuses and the step runs RoPE + append + the generic attention on its own"""
    B, H, hd, maxS = 1, 2, 128, 12288
    g = torch.Generator(device="cuda").manual_seed(11 + t)
    tab_d = rope_table(lib, maxS, hd).cuda()
    scale = hd ** -0.5
    mut = []
    for pos in ([maxS - 1], [4000], [300]):
        qkv = torch.randn(B, 3 * H * hd, device="cuda", generator=g)
        kc0, vc0 = _rand_cache(B, maxS, H, hd, t, g), _rand_cache(B, maxS, H, hd, t, g)
        kc, vc = kc0.clone(), vc0.clone()
        pos_d = torch.tensor(pos, dtype=torch.int32, device="cuda")
        out = torch.full((B, H * hd), float("nan"), device="cuda")
        check(lib, lib.anyref_op_decode_attn(t, None, P(qkv), B, H, hd, P(pos_d), P(tab_d), P(kc), P(vc), maxS, scale,
                                             P(out), None, 0))
        keep = torch.ones(B, maxS, dtype=torch.bool, device="cuda")
        keep[0, pos[0]] = False
        assert torch.equal(kc[keep], kc0[keep]) and torch.equal(vc[keep], vc0[keep])
        x = qkv.view(B, 3, H, hd)
        cs, sn = tab_d[pos[0], 0][None, None], tab_d[pos[0], 1][None, None]
        qr, _ = rotate64(x[:, 0, :, :64], x[:, 0, :, 64:], cs, sn)
        q = qr.to(_DT[t]).float()          # the fallback's q as rope_cache stores it (round to nearest of the f32 value)
        o, pv, dt = decode_reference(q, kc, vc, pos, H, hd, scale)
        # the f32 rotation may round q to the neighbouring T value: one ulp of q moves the scores by ulp |k| scale
        dq = torch.einsum("hd,nhd->hn", ulp(qr[0], t), kc[0, : pos[0] + 1].double().abs()) * scale
        pr = torch.softmax(torch.einsum("hd,nhd->hn", qr[0], kc[0, : pos[0] + 1].double()) * scale, -1)
        dt = dt + (torch.einsum("hn,nhd->hd", pr * dq, vc[0, : pos[0] + 1].double().abs())
                   + (pr * dq).sum(-1, keepdim=True) * o[0].abs())[None]
        bound = decode_bound(pv, dt, o, pos, t, hd, True)
        r = ((out.view(B, H, hd).double() - o).abs() / bound).max().item()
        assert r <= 1.0, f"long-cache fallback: worst error / bound = {r:.3f}"
        # mutant: the generic kernel's last key tile (32 keys f32 / 64 bf16) left out -- among 4000+ keys a bf16 tile is
        # ~1.5 % of the weight and sits inside the 2^-8 of the rounded P (measured: 0.37 of the bound); at p = 300 it is not
        om, _, _ = decode_reference(q, kc, vc, pos, H, hd, scale, drop=64 if t == 1 else 32)
        mut.append(((om - o).abs() / bound).max().item())
        print(f"decode_attn long cache t={t} p={pos[0]}: worst error / bound {r:.3g}, mutant {mut[-1]:.3g}")
    assert max(mut) > 1, f"long-cache fallback: a dropped key tile stays inside the bound ({max(mut):.3f})"


# ----------------------------------------------------------------------------------------------------------------------
# Prefill RoPE + KV append
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bf16_vec", "bf16_scalar", "f32_scalar", "slabs_bf16", "slabs_f32"])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_cache(lib, form, hd):
    """launch_rope_cache / launch_rope_cache_slabs: ragged lens, nonzero pos0.  q_out and the appended cache / q_keep rows
    within 1 ulp of T of the float64 rotation, v exactly T(v); rows >= lens[b] of q_out and every other cache row
    bitwise unchanged.  bf16_scalar: the qkv buffer 2 bytes off 16-byte alignment takes rope_cache_kernel<bf16, bf16>."""
    t = 0 if form in ("f32_scalar", "slabs_f32") else 1
    B, S, H, maxS = 3, 37, 4, 160
    lens, pos0 = [S, S - 9, 1], [0, 23, maxS - S]
    g = torch.Generator(device="cuda").manual_seed(hd + len(form))
    tab_d = rope_table(lib, maxS, hd).cuda()
    n = B * S * 3 * H * hd
    slab0 = slab1 = qkv = None
    if form.startswith("slabs"):
        slab0 = torch.randn(n, device="cuda", generator=g)
        slab1 = torch.randn(n, device="cuda", generator=g) * 0.25
        xin = (slab0 + slab1)                         # the kernel's f32 add
        xin = xin.to(_DT[t]).float() if t == 1 else xin
    else:
        raw = torch.randn(n + 8, device="cuda", generator=g).to(_DT[t])
        qkv = raw[1: n + 1] if form == "bf16_scalar" else raw[:n]
        assert (qkv.data_ptr() % 16 != 0) == (form == "bf16_scalar")
        xin = qkv.float()
    x = xin.view(B, S, 3, H, hd)
    q_out0 = (torch.randn(B, S, H, hd, device="cuda", generator=g)).to(_DT[t])
    kc0, vc0, qk0 = (_rand_cache(B, maxS, H, hd, t, g) for _ in range(3))
    q_out, kc, vc, qk = q_out0.clone(), kc0.clone(), vc0.clone(), qk0.clone()
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    pos0_d = torch.tensor(pos0, dtype=torch.int32, device="cuda")
    check(lib, lib.anyref_op_rope_cache(t, None, P(qkv), P(slab0), P(slab1), B, S, H, hd, P(pos0_d), P(lens_d), P(tab_d),
                                        P(q_out), P(kc), P(vc), maxS, P(qk)))
    half = hd // 2
    written = torch.zeros(B, maxS, dtype=torch.bool, device="cuda")
    qrow = torch.zeros(B, S, dtype=torch.bool, device="cuda")
    for b in range(B):
        L, p0 = lens[b], pos0[b]
        written[b, p0: p0 + L] = True
        qrow[b, :L] = True
        cs, sn = tab_d[p0: p0 + L, 0][:, None], tab_d[p0: p0 + L, 1][:, None]
        qr, eq = rotate64(x[b, :L, 0, :, :half], x[b, :L, 0, :, half:], cs, sn)
        kr, ek = rotate64(x[b, :L, 1, :, :half], x[b, :L, 1, :, half:], cs, sn)
        assert_rounded(q_out[b, :L], qr, eq, t, f"{form} q_out")
        assert_rounded(qk[b, p0: p0 + L], qr, eq, t, f"{form} q_keep")
        assert_rounded(kc[b, p0: p0 + L], kr, ek, t, f"{form} kc")
        assert torch.equal(vc[b, p0: p0 + L], x[b, :L, 2].to(_DT[t])), f"{form}: v row is not v rounded to T"
        assert torch.equal(q_out[b, :L], qk[b, p0: p0 + L]), f"{form}: q_keep differs from q_out"
    for name, new, old, m in (("q_out", q_out, q_out0, ~qrow), ("kc", kc, kc0, ~written), ("vc", vc, vc0, ~written),
                              ("q_keep", qk, qk0, ~written)):
        assert torch.equal(new[m], old[m]), f"{form}: {name} changed outside the appended rows"


# ----------------------------------------------------------------------------------------------------------------------
# argmax (greedy token) and its decode-step form
# ----------------------------------------------------------------------------------------------------------------------
def _argmax_rows(N, M, g):
    """M rows of values in [-1, 1) with maxima (value 2) placed to tie inside one float4, across lanes of one wave,
    the same lane in two unrolled loads, across waves, between the vector body and the scalar tail, everywhere"""
    x = torch.rand(M, N, generator=g) * 2 - 1
    n4 = N // 4
    places = [
        [],                                           # a unique random maximum
        [4 * 3 + 2, 4 * 3 + 1],                       # one float4
        [4 * 50, 4 * 3 + 3],                          # lanes 3 and 50 of wave 0
        [4 * (7 + 1024), 4 * 7 + 1],                  # lane 7, loads u = 1 and u = 0
        [4 * 900 + 1, 4 * 100 + 2],                   # waves 14 and 1
        [N - 1, 4 * n4 - 1],                          # scalar tail and the last vector element
        [N - 1],                                      # only in the tail (or the last element)
        [N - 1, 0],                                   # first and last element
        list(range(N)),                               # every element
        [4 * 8191 + 3, 4 * 5000],                     # the last float4 of a 32k row and one before
        [N - 2, N - 1],
        [4 * 1023 + 3, 4 * 1024],                     # the last lane of the last wave and lane 0 of the next load
    ]
    for r in range(M):
        for i in places[r % len(places)]:
            if 0 <= i < N:
                x[r, i] = 2.0
    return x


@pytest.mark.parametrize("N", [1, 3, 5, 1000, 32000, 32001, 32007])
@pytest.mark.parametrize("aligned", [1, 0])
def test_argmax(lib, N, aligned):
    """first index of the maximum, as torch.argmax, on the vector path (ldx % 4 == 0, aligned rows) and the scalar one"""
    M = 12
    g = torch.Generator().manual_seed(N + aligned)
    x = _argmax_rows(N, M, g)
    ldx = (N + 3) // 4 * 4 + 4 if aligned else (N + 3) // 4 * 4 + 1
    buf = torch.full((M, ldx), 5.0)                  # padding beyond N larger than every entry: must not be read
    buf[:, :N] = x
    xd = buf.cuda()
    out = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    pos = torch.arange(M, dtype=torch.int32, device="cuda") * 3
    check(lib, lib.anyref_op_argmax(None, P(xd), M, N, ldx, P(out), P(pos), None, 0, 0, 0, None, None, None))
    assert torch.equal(out.cpu(), torch.argmax(x, -1)), (out.cpu(), torch.argmax(x, -1))
    assert torch.equal(pos.cpu(), torch.arange(M, dtype=torch.int32) * 3 + 1), "pos not bumped by one"


@pytest.mark.parametrize("N", [5, 1000, 32001])
@pytest.mark.parametrize("aligned", [1, 0])
def test_argmax_nan_and_minus_inf_rows(lib, N, aligned):
    """rows of NaN and -inf (through the plain form only: it writes out[b] and nothing else): NaN counts as the greatest
    value, the first NaN is returned as torch does; an all -inf row gives 0; every index lies in [0, N)"""
    inf, nan = float("inf"), float("nan")
    rows = []
    r = torch.full((N,), -inf); rows.append(r)                                   # all -inf -> 0
    r = torch.full((N,), nan); rows.append(r)                                    # all NaN -> 0
    r = torch.rand(N) - 0.5; r[N // 2] = nan; r[N - 1] = nan; r[1] = inf; rows.append(r)   # first NaN, not the +inf
    r = torch.rand(N) - 0.5; r[N - 1] = nan; rows.append(r)                      # NaN in the scalar tail / last
    r = torch.full((N,), -inf); r[N - 1] = 0.0; rows.append(r)                   # -inf everywhere but the last
    r = torch.rand(N) - 0.5; r[3] = nan; r[0] = nan; rows.append(r)              # two NaN: the first
    x = torch.stack(rows)
    M = x.shape[0]
    ldx = (N + 3) // 4 * 4 if aligned else (N + 3) // 4 * 4 + 1
    buf = torch.zeros(M, ldx)
    buf[:, :N] = x
    out = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    check(lib, lib.anyref_op_argmax(None, P(buf.cuda()), M, N, ldx, P(out), None, None, 0, 0, 0, None, None, None))
    got = out.cpu()
    assert ((got >= 0) & (got < N)).all(), got
    assert torch.equal(got, torch.tensor([0, 0, N // 2, N - 1, N - 1, 0])), got
    assert torch.equal(got, torch.argmax(x, -1)), (got, torch.argmax(x, -1))


@pytest.mark.parametrize("is_bf16", [1, 0])
@pytest.mark.parametrize("N,D", [(32007, 4096), (1000, 320)])
def test_argmax_next(lib, is_bf16, N, D):
    """launch_argmax_next: the chosen id, pos + 1, row_map = b * maxS + pos, kvlen = pos + 1 and x_next = the widened
    embedding row of the chosen id, bit for bit"""
    M, maxS = 12, 640
    g = torch.Generator().manual_seed(N + D + is_bf16)
    x = _argmax_rows(N, M, g)
    table = torch.randn(N, D, generator=g)
    table = table.to(torch.bfloat16) if is_bf16 else table
    pos0 = torch.randint(0, maxS - 1, (M,), generator=g, dtype=torch.int32)
    pos = pos0.cuda()
    out = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    x_next = torch.full((M, D), float("nan"), device="cuda")
    row_map = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    kvlen = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    check(lib, lib.anyref_op_argmax(None, P(x.cuda()), M, N, N, P(out), P(pos), P(table.cuda()), is_bf16, D, maxS,
                                    P(x_next), P(row_map), P(kvlen)))
    ids = torch.argmax(x, -1)
    assert torch.equal(out.cpu(), ids)
    p1 = pos0 + 1
    assert torch.equal(pos.cpu(), p1)
    assert torch.equal(row_map.cpu(), torch.arange(M, dtype=torch.int32) * maxS + p1)
    assert torch.equal(kvlen.cpu(), p1 + 1)
    assert torch.equal(x_next.cpu(), table[ids].float())


# ----------------------------------------------------------------------------------------------------------------------
# lm_head GEMV: the f32 normalised rows (hidden_states[-1] of each decode position)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("B", [1, 4, 8])
def test_gemv_xn_rows(lib, t, B):
    """xn_out[row_map[b]] = rmsnorm(x[b]) * gain in f32 (the [SEG] hidden state SAM receives): the mapped rows within the
    f32 norm bound of test_norm (2e-5 of max(1, max|ref|)), every other row bitwise unchanged.  B = 8 (bf16) is
    gemv_rows8_kernel."""
    N, K, R, ld = 32007, 4096, 30, 4096 + 8
    g = torch.Generator().manual_seed(B * 5 + t)
    x = torch.randn(B, K, generator=g) * 2 + 0.5
    gain = 1 + 0.1 * torch.randn(K, generator=g)
    W = (torch.randn(N, K, generator=g) * 0.05).to(_DT[t])
    rmap = torch.randperm(R, generator=g)[:B].to(torch.int32)
    xn0 = torch.randn(R, ld, generator=g)
    xn = xn0.cuda()
    y = torch.empty(B, N, device="cuda")
    check(lib, lib.anyref_op_gemv_xn(t, None, P(x.cuda()), P(gain.cuda()), 1e-6, P(W.cuda()), None, None, P(y), None, B, N,
                                     K, 0, P(xn), P(rmap.cuda()), ld))
    xd = x.double()
    ref = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * gain.double()
    got = xn.cpu()
    err = (got[rmap.long(), :K].double() - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert err <= 2e-5 * scale, f"xn rows: max abs err {err:.3e} (scale {scale:.3e})"
    other = torch.ones(R, dtype=torch.bool)
    other[rmap.long()] = False
    assert torch.equal(got[other], xn0[other]), "xn_out rows outside the row map changed"
    assert torch.equal(got[rmap.long(), K:], xn0[rmap.long(), K:]), "xn_out written beyond K"
    # y: the products of the (T-rounded) normalised rows; the f32 sum over K within 2^-24 (K/32 + 16) sum |x w|
    # plus the bf16 rounding of the staged rows (a flip either way: 2^-8 |xn| |w|)
    # and the f32 normalisation itself (a few units of 2^-24 of |xn|)
    ref, Wd = ref.cuda(), W.cuda().double()
    xr = ref.to(_DT[t]).double() if t == 1 else ref
    yref = xr @ Wd.t()
    bnd = ((K / 32 + 16) * U32 * xr.abs() + 8 * U32 * ref.abs()) @ Wd.abs().t()
    if t == 1:
        bnd = bnd + _flip_term(ref, Wd)
    r = ((y.double() - yref).abs() / bnd).max().item()
    assert r <= 1.0, f"lm_head y: worst error / bound = {r:.3f}"


def _flip_term(ref, W):
    """an f32 normalised value within 2^-17 (relative) of a bf16 rounding boundary may round either way: such entries
    contribute their rounding step |up - down| * |w|"""
    lo, hi = (ref * (1 - 2.0 ** -17)).to(torch.bfloat16).double(), (ref * (1 + 2.0 ** -17)).to(torch.bfloat16).double()
    return (hi - lo).abs() @ W.abs().t()
