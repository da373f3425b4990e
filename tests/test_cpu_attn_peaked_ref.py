"""Proves tests/attn_peaked_ref.py without a GPU, for every case tests/test_gpu_attn_peaked.py runs, at the same shape and
seed: the inputs reach the softmax rescale paths (conditions on the emulation's own counters), the f32 emulation in the
kernels' order lies inside the float64 bound, every mutant lies outside it -- and the inputs of test_gpu_ops.test_attention
never move the reference maximum after the first tile, which is why the peaked cases exist."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_peaked_ref as A  # noqa: E402
import gemm_forms_ref as R  # noqa: E402
import test_gpu_decode_ops as D  # noqa: E402
import test_gpu_f16_ops as F  # noqa: E402
import test_gpu_ops as G  # noqa: E402

COMBOS = [(c, ty, pr, b) for c in A.CASES for ty in c.tys for pr in c.profiles for b in c.biases]
_ID = lambda v: v.name if isinstance(v, A.Case) else str(v)      # noqa: E731


def test_randn_inputs_never_move_the_reference():
    """the counter of attention_kernel_order over the inputs of test_gpu_ops.test_attention (its seed formula, bf16 and f16
    roundings, tile widths as dispatched, one stream of tiles per row): zero moves after the first tile in all 14 cases"""
    cases = [m for m in G.test_attention.pytestmark if m.name == "parametrize" and "Sq" in m.args[0]][0].args[1]
    assert len(cases) == 14
    for ty in (1, 2):
        for B, H, Sq, Sk, hd, causal in cases:
            g = torch.Generator().manual_seed(Sq * 3 + Sk + hd)
            q, k, v = (R.rnd(torch.randn(B, S, H, hd, generator=g), ty) for S in (Sq, Sk, Sk))
            kv_len = [Sk - 7 * b for b in range(B)] if B > 1 and Sk > 64 and not causal else None
            w = 64
            if hd == 80 and Sq == Sk and 192 < Sq <= 240 and not causal:
                w = 48 if (Sq <= 208 and kv_len is None) else 80
            st = A.new_stats()
            A.attention_kernel_order(ty, q, k, v, hd ** -0.5, A.key_ranges(Sk, w), stats=st,
                                     mask=A.key_mask(B, Sq, Sk, q.device, causal=bool(causal), kv_len=kv_len))
            assert st["moves"] == 0 and st["max_p"] <= 2 ** A.LAZY, (ty, B, H, Sq, Sk, hd, causal, st)
            assert st["events"] > 0 or Sk <= w


@pytest.mark.parametrize("case,ty,profile,bias", COMBOS, ids=_ID)
def test_peaked_attention(case, ty, profile, bias):
    x = A.case_inputs(case, ty, profile, bias)
    ref_kw, emu_kw = A.form_kwargs(case, x, ty, bias, x["q"].device)
    ref, bound = R.attention_form(ty, x["q"], x["k"], x["v"], x["scale"], **ref_kw)
    st = A.new_stats()
    emu = A.attention_kernel_order(ty, x["q"], x["k"], x["v"], x["scale"], x["ranges"], stats=st, **emu_kw)
    print(f"{case.name} t={ty} {profile} bias={bias} w={x['w']}: {st}")
    # ---- coverage of the input ----
    stairs = profile in ("stairs", "stairs_mid")
    if ty != 0:
        assert st["max_p"] <= 2 ** A.LAZY * (1 + 2.0 ** -20), st
        if stairs and case.name != "split9":      # (split9: one step per key split -- its moves are the merge's, below)
            assert st["moves"] >= 0.1 * st["events"] and st["lazy_gt1"] >= 0.1 * st["events"], st
            assert st["max_p"] >= 100, st
            assert st["mixed"], st
    if case.name != "g2":      # the key splits emulated are the ones the launcher's rule gives this shape
        B, H, Sq, Sk, _ = case.dims
        assert A.kv_splits(B, H, Sq, Sk, case.causal, case.kv_len is not None, A.query_block(case)) == case.splits
    if A.case_splits(case, ty) > 1:
        assert st["split_gap"] >= A.LAZY * (1 if ty else 1 / A.LOG2E), st      # 8 log2 units (t = 0 counts in natural ones)
    # ---- the emulation inside, every mutant outside ----
    muts = {n: A.attention_kernel_order(ty, x["q"], x["k"], x["v"], x["scale"], x["ranges"], mutant=n, **emu_kw)
            for n in A.mutant_names(case, ty, profile)}
    muts["drop_tile"] = R.attention_form(ty, x["q"], x["k"], x["v"], x["scale"], loss="drop_tile", **ref_kw)[0]
    R.check_bound(emu, ref, bound, muts, f"cpu peaked attention {case.name} t={ty} {profile} bias={bias}")
    if A.case_splits(case, ty) > 1:
        eq = A.attention_kernel_order(ty, x["q"], x["k"], x["v"], x["scale"], x["ranges"], mutant=A.SPLIT_EQUIVALENT, **emu_kw)
        print(f"  {A.SPLIT_EQUIVALENT} (an equivalent merge): error / bound {R.ratio(eq, ref, bound):.3g}")


@pytest.mark.parametrize("ty", A.EMPTY.tys)
def test_empty_rows(ty):
    """kv_len = 0: l_run stays 0 and inv = l_run > 0 ? 1 / l_run : 0 writes exact zeros; the other batch element is ordinary"""
    case = A.EMPTY
    x = A.case_inputs(case, ty, "stairs", None)
    _, emu_kw = A.form_kwargs(case, x, ty, None, x["q"].device)
    emu = A.attention_kernel_order(ty, x["q"], x["k"], x["v"], x["scale"], x["ranges"], **emu_kw)
    assert torch.equal(emu[0], torch.zeros_like(emu[0]))
    ref, bound = R.attention_form(ty, x["q"][1:], x["k"][1:], x["v"][1:], x["scale"], kv_len=case.kv_len[1:], tile=x["w"])
    mut = R.attention_form(ty, x["q"][1:], x["k"][1:], x["v"][1:], x["scale"], kv_len=case.kv_len[1:], tile=x["w"],
                           loss="drop_tile")[0]
    R.check_bound(emu[1:], ref, bound, {"drop_tile": mut}, f"cpu empty rows t={ty}")


@pytest.mark.parametrize("profile", A.DECODE_PROFILES)
@pytest.mark.parametrize("hd,H", A.DECODE_CFG)
@pytest.mark.parametrize("t", [0, 1, 2])
def test_peaked_decode(t, hd, H, profile):
    pos = A.decode_positions(t, hd)
    tab = A.rope_table64(A.DECODE_MAXS, hd)
    scale = hd ** -0.5
    qkv, kc0, vc0, qk0 = A.decode_inputs(t, hd, H, pos, profile, tab, D.rotate64)
    kc, vc, qk = A.decode_append(t, qkv, pos, tab, kc0, vc0, qk0)
    bi, pd = torch.arange(len(pos)), torch.tensor(pos)
    q = qk[bi, pd].float()
    o, pv, dt = D.decode_reference(q, kc, vc, pos, H, hd, scale)
    om = D.decode_reference(q, kc, vc, pos, H, hd, scale, drop=1)[0]
    keep = torch.tensor([p > 0 for p in pos])
    for fb in (0, 1):
        bound = F.decode_bound16(pv, dt, o, pos, hd, fb) if t == 2 else D.decode_bound(pv, dt, o, pos, t, hd, fb)
        if fb == 0:
            st = dict(group_gap=0.0, batch_rise=0.0)
            emu = A.decode_kernel_order(t, q, kc, vc, pos, scale, stats=st)
            print(f"decode t={t} hd={hd} {profile}: {st}")
            if profile != "stairs":
                assert st["group_gap"] >= 20, st
            if profile == "spike_self":
                assert st["batch_rise"] >= 8, st
            if profile == "stairs":      # a stair is 7 natural units, the noise of the keys about 0.5
                assert st["batch_rise"] >= 6, st
            muts = {n: A.decode_kernel_order(t, q, kc, vc, pos, scale, mutant=n) for n in A.DECODE_MUTANTS}
        else:      # the fallback: the generic attention with one query row over the cache, kv_len = p + 1
            w = 32 if t == 0 else 64
            kw = dict(mask=A.key_mask(len(pos), 1, A.DECODE_MAXS, q.device, kv_len=[p + 1 for p in pos]), o_f32=True)
            args = (t, q[:, None], kc.float(), vc.float(), scale, A.key_ranges(A.DECODE_MAXS, w))
            emu = A.attention_kernel_order(*args, **kw)[:, 0]
            muts = {n: A.attention_kernel_order(*args, mutant=n, **kw)[:, 0] for n in A.MUTANTS[:2] if profile != "sink"}
        assert R.ratio(om[keep], o[keep], bound[keep]) > 1, "bound too loose to see a dropped appended key"
        R.check_bound(emu, o, bound, muts, f"cpu peaked decode t={t} hd={hd} {profile} fallback={fb}")
