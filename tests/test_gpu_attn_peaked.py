"""Attention kernels on peaked scores (tests/attn_peaked_ref.py): every launch form of attention.hip through
anyref_op_attention_ex and the decode step through anyref_op_decode_attn, on inputs whose running maximum keeps moving
between key tiles -- the lazy rescale of the 16-bit / split-pair bodies, the merge of the key-split partials and of the
decode kernel's lane groups, P underflow behind a sink, and rows without any key.  References and bounds: float64
(gemm_forms_ref.attention_form, test_gpu_decode_ops.decode_reference / decode_bound); mutants: the f32 emulation in the
kernels' order with one rescale lost (proved on the CPU by tests/test_cpu_attn_peaked_ref.py).  Every case asserts the
tag of the form it ran; outputs start as a sentinel that unwritten rows must keep."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_peaked_ref as A  # noqa: E402
import gemm_forms_ref as R  # noqa: E402
import test_gpu_decode_ops as D  # noqa: E402
import test_gpu_f16_ops as F  # noqa: E402
from test_gpu_gemm_forms import adt, attn_ex  # noqa: E402
from test_gpu_ops import P, check  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = [(c, ty, b) for c in A.CASES for ty in c.tys for b in c.biases]
_ID = lambda v: v.name if isinstance(v, A.Case) else str(v)      # noqa: E731


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device="cuda")


def run_case(lib, case, ty, x, bias, cap):
    """one launch over the stored operands of x; returns (o [B, Sq, H, hd] as stored, tags)"""
    B, H, Sq, Sk, hd = case.dims
    dt = adt(ty)
    q = x["q"].cuda().to(dt).contiguous()
    rows = case.maxS or Sk
    g = torch.Generator().manual_seed(Sk)
    k, v = ((torch.randn(B, rows, H, hd, generator=g) * 3).cuda().to(dt) for _ in range(2))      # cache rows past Sk: noise
    k[:, :Sk], v[:, :Sk] = x["k"].cuda().to(dt), x["v"].cuda().to(dt)
    o_rs = -(-H * hd // 64) * 64                      # whole pair rows (t = 3); the padding must keep the sentinel too
    o = torch.full((B, Sq, o_rs), A.SENT, dtype=dt, device="cuda")
    kw = dict(q=q, k=k, v=v, o=o, q_bs=Sq * H * hd, q_rs=H * hd, q_hs=hd, k_bs=rows * H * hd, k_rs=H * hd, k_hs=hd,
              v_bs=rows * H * hd, v_rs=H * hd, v_hs=hd, o_bs=Sq * o_rs, o_rs=o_rs, o_hs=hd, B=B, H=H, Sq=Sq, Sk=Sk, hd=hd,
              scale=x["scale"], causal=case.causal, max_wg=cap)
    keep = [i32(case.q_len), i32(case.kv_len), i32(case.q_pos0)]
    for name, t in zip(("q_len", "kv_len", "q_pos0"), keep):
        if t is not None:
            kw[name] = t
    size = x["size"]
    if bias == "tab":
        ld = 128
        tab = torch.zeros(2, 2 * size, ld, device="cuda")
        tab[0, : 2 * size - 1, :hd], tab[1, : 2 * size - 1, :hd] = x["th"].cuda(), x["tw"].cuda()
        tab = tab.to(dt)
        kw.update(rel_tab_h=tab[0], rel_tab_w=tab[1], rel_tab_ld=ld, kh=size, kw=size)
    elif bias == "p":
        npad = 2 * size
        p = torch.zeros(H, B * Sq, 2 * npad, device="cuda")
        qh = q.float().permute(2, 0, 1, 3).reshape(H, B * Sq, hd)
        p[:, :, : 2 * size - 1] = qh @ x["th"].cuda().t()
        p[:, :, npad: npad + 2 * size - 1] = qh @ x["tw"].cuda().t()
        kw.update(rel_p=p, rel_ld=2 * npad, rel_hs=B * Sq * 2 * npad, kh=size, kw=size)
    tags = attn_ex(lib, ty, **kw)
    assert torch.equal(o[..., H * hd:], torch.full_like(o[..., H * hd:], A.SENT)), "the padding of the o rows was written"
    return o[..., : H * hd].reshape(B, Sq, H, hd), tags


@pytest.mark.parametrize("case,ty,bias", COMBOS, ids=_ID)
def test_peaked_attention(lib, case, ty, bias):
    pre, sub = A.want_tag(case, ty, bias)
    for profile in case.profiles:
        x = A.case_inputs(case, ty, profile, bias)
        outs = []
        for cap in case.caps:
            o, tags = run_case(lib, case, ty, x, bias, cap)
            assert tags == [pre + sub], (pre + sub, tags)
            outs.append(o)
        for o in outs[1:]:
            assert torch.equal(outs[0], o), "max_wg changes the result"
        qd, kd, vd = (x[n].cuda() for n in "qkv")
        ref_kw, emu_kw = A.form_kwargs(case, x, ty, bias, "cuda")
        ref, bound = R.attention_form(ty, qd, kd, vd, x["scale"], **ref_kw)
        muts = {n: A.attention_kernel_order(ty, qd, kd, vd, x["scale"], x["ranges"], mutant=n, **emu_kw)
                for n in A.mutant_names(case, ty, profile)}
        muts["drop_tile"] = R.attention_form(ty, qd, kd, vd, x["scale"], loss="drop_tile", **ref_kw)[0]
        R.check_bound(outs[0], ref, bound, muts, f"peaked attention {case.name} t={ty} {profile} bias={bias} [{tags[0]}]")


@pytest.mark.parametrize("ty", A.EMPTY.tys)
def test_rows_without_keys(lib, ty):
    """kv_len = [0, 70], not causal: batch element 0 has no key at all -- l_run stays 0, the row is written as exact zeros
    (inv = l_run > 0 ? 1 / l_run : 0), no NaN; batch element 1 stays inside its bound"""
    case = A.EMPTY
    x = A.case_inputs(case, ty, "stairs", None)
    o, tags = run_case(lib, case, ty, x, None, 0)
    assert tags == [A.TAG[ty] + "64"], tags
    assert torch.isfinite(o.float()).all()
    assert torch.equal(o[0].float(), torch.zeros_like(o[0].float())), "rows without keys are not exact zeros"
    qd, kd, vd = (x[n][1:].cuda() for n in "qkv")
    kw = dict(kv_len=case.kv_len[1:], tile=x["w"])
    ref, bound = R.attention_form(ty, qd, kd, vd, x["scale"], **kw)
    mut = R.attention_form(ty, qd, kd, vd, x["scale"], loss="drop_tile", **kw)[0]
    R.check_bound(o[1:], ref, bound, {"drop_tile": mut}, f"rows without keys t={ty}, the other batch element [{tags[0]}]")


@pytest.mark.parametrize("hd,H", A.DECODE_CFG)
@pytest.mark.parametrize("t", [0, 1, 2])
def test_peaked_decode(lib, t, hd, H):
    """decode_attn_kernel and its fallback over a cache whose keys follow a score profile along this step's rotated q:
    stairs (a step per key batch: every lane group's running maximum rises batch after batch), sink (key 0: one lane group
    far above the others at the merge), spike_self (the appended key, taken from LDS, is the peak).  The checks of
    test_decode_attn stay: row p within 1 ulp, every other row bitwise unchanged, the dropped appended key outside."""
    maxS = A.DECODE_MAXS
    tab = D.rope_table(lib, maxS, hd)
    tab_d = tab.cuda()
    scale = hd ** -0.5
    pos = A.decode_positions(t, hd)
    B = len(pos)
    pos_d = i32(pos)
    bi, pd = torch.arange(B, device="cuda"), pos_d.long()
    for profile in A.DECODE_PROFILES:
        qkv, kc0, vc0, qk0 = (y.cuda() for y in A.decode_inputs(t, hd, H, pos, profile, tab, D.rotate64))
        for fb in (0, 1):
            kc, vc, qk = kc0.clone(), vc0.clone(), qk0.clone()
            out = torch.full((B, H * hd), float("nan"), device="cuda")
            check(lib, lib.anyref_op_decode_attn(t, None, P(qkv), B, H, hd, P(pos_d), P(tab_d), P(kc), P(vc), maxS, scale,
                                                 P(out), P(qk), fb))
            for name, new, old in (("kc", kc, kc0), ("vc", vc, vc0), ("q_keep", qk, qk0)):
                keep = torch.ones(B, maxS, dtype=torch.bool, device="cuda")
                keep[bi, pd] = False
                assert torch.equal(new[keep], old[keep]), f"{name}: a row other than the appended one changed"
            xq = qkv.view(B, 3, H, hd)
            cs, sn = tab_d[pd, 0][:, None, :], tab_d[pd, 1][:, None, :]
            half = hd // 2
            for name, j, buf in (("q_keep", 0, qk), ("kc", 1, kc)):
                ref, e32 = D.rotate64(xq[:, j, :, :half], xq[:, j, :, half:], cs, sn)
                if t == 2:
                    F.assert_rounded16(buf[bi, pd], ref, e32, f"{name} row p (fallback={fb})")
                else:
                    D.assert_rounded(buf[bi, pd], ref, e32, t, f"{name} row p (fallback={fb})")
            assert torch.equal(vc[bi, pd], xq[:, 2].to(A.DECODE_DT[t])), "vc row p is not v rounded to T"
            q = qk[bi, pd].float()
            o, pv, dt = D.decode_reference(q, kc, vc, pos, H, hd, scale)
            bound = F.decode_bound16(pv, dt, o, pos, hd, fb) if t == 2 else D.decode_bound(pv, dt, o, pos, t, hd, fb)
            om = D.decode_reference(q, kc, vc, pos, H, hd, scale, drop=1)[0]
            keep_b = torch.tensor([p > 0 for p in pos], device="cuda")
            assert R.ratio(om[keep_b], o[keep_b], bound[keep_b]) > 1, "bound too loose to see a dropped appended key"
            if fb == 0:
                muts = {n: A.decode_kernel_order(t, q, kc, vc, pos, scale, mutant=n) for n in A.DECODE_MUTANTS}
            else:
                args = (t, q[:, None], kc.float(), vc.float(), scale, A.key_ranges(maxS, 32 if t == 0 else 64))
                kw = dict(mask=A.key_mask(B, 1, maxS, "cuda", kv_len=[p + 1 for p in pos]), o_f32=True)
                muts = {n: A.attention_kernel_order(*args, mutant=n, **kw)[:, 0] for n in A.MUTANTS[:2] if profile != "sink"}
            R.check_bound(out.view(B, H, hd), o, bound, muts, f"peaked decode t={t} hd={hd} {profile} fallback={fb}")
