"""Kernel-level tests of the two spatial-prompt kernels (anyref_amd/csrc/prompt_encode.hip) through anyref_op_prompt_tokens /
anyref_op_mask_prompt_embed, and of the two f32 attention forms the prompted decoder adds (10 queries instead of 6) through the
existing anyref_op_attention.  References, bounds, mutants and shapes: tests/prompt_ops_ref.py (proved on the CPU by
tests/test_cpu_prompt_ops_ref.py).  Outputs live in buffers prefilled with a NaN bit pattern with guard rows behind them; a
refused call must leave the pattern; a rerun must give the same bits."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ops_ref as R  # noqa: E402
import gemm_forms_ref as G  # noqa: E402
import prompt_ops_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 2


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def cu(t):
    return None if t is None else t.cuda().contiguous()


def ok(lib, rc):
    assert rc == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()


def guards_intact(buf, rows, what):
    pat = R.bits(R.nan_fill(buf.shape, buf.dtype, "cuda"))
    n = int((R.bits(buf)[rows:] != pat[rows:]).sum())
    assert n == 0, f"{what}: {n} guard words were written"


def untouched(buf):
    return bool((R.bits(buf) == R.bits(R.nan_fill(buf.shape, buf.dtype, "cuda"))).all())


# ---- prompt_tokens ---------------------------------------------------------------------------------------------------
def run_tokens(lib, c, n, C_, out, *, max_wg=0, over=None):
    a = dict(out_tokens=cu(c["out_tokens"]), points=cu(c["points"]), labels=cu(c["labels"]), boxes=cu(c["boxes"]),
             text=cu(c["text"]), gauss=cu(c["gauss"]), emb5=cu(c["emb5"]), n=n, C=C_,
             P=0 if c["points"] is None else c["points"].shape[1])
    a.update(over or {})
    rc = lib.anyref_op_prompt_tokens(None, ptr(a["out_tokens"]), PR.TOKEN_N_OUT, ptr(a["points"]), ptr(a["labels"]), a["P"],
                                     ptr(a["boxes"]), ptr(a["text"]), ptr(a["gauss"]), ptr(a["emb5"]), a["n"], a["C"], c["S"],
                                     ptr(out), max_wg)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", PR.TOKEN_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_prompt_tokens(lib, case):
    n, P, box, text, C_ = case
    c = PR.token_case(*case)
    rows = n * PR.token_rows(PR.TOKEN_N_OUT, P, box, text)
    what = f"prompt_tokens {case}"
    outs = []
    for max_wg in (0, 2):                 # 2 workgroups: 30 rows x 64 threads take the grid-stride loop
        out = R.nan_fill((rows + GUARD, C_), device="cuda")
        ok(lib, run_tokens(lib, c, n, C_, out, max_wg=max_wg))
        R.check_bound(out[:rows].reshape(c["ref"].shape), c["ref"].cuda(), c["bound"].cuda(), c["mutants"], what)
        guards_intact(out, rows, what)
        exact = (c["bound"] == 0).cuda()
        got = out[:rows].reshape(c["ref"].shape)
        assert (R.bits(got)[exact] == R.bits(c["ref"].float().cuda())[exact]).all(), f"{what}: a copied row is not bit for bit"
        outs.append(out)
    assert torch.equal(R.bits(outs[0]), R.bits(outs[1])), f"{what}: the capped grid gives other bits"
    again = R.nan_fill((rows + GUARD, C_), device="cuda")
    ok(lib, run_tokens(lib, c, n, C_, again))
    assert torch.equal(R.bits(again), R.bits(outs[0])), f"{what}: a rerun gives other bits"


def test_prompt_tokens_refusals(lib):
    case = PR.TOKEN_CASES[1]
    n, P, box, text, C_ = case
    c = PR.token_case(*case)
    out = R.nan_fill((n * 16 + GUARD, C_), device="cuda")
    for over in (dict(C=12), dict(C=4), dict(n=0), dict(labels=None), dict(points=None), dict(P=-1), dict(gauss=None)):
        rc = run_tokens(lib, c, n, C_, out, over=over)
        assert rc != 0 and lib.anyref_op_last_error().decode(), f"accepted {over}"
        assert untouched(out), f"a refused call ({over}) wrote to its output"


# ---- mask_prompt_embed -----------------------------------------------------------------------------------------------
def run_embed(lib, c, n, g, C_, c1, c2, out, *, max_wg=0):
    W = {k: cu(v) for k, v in c["W"].items()}
    mask, emb = cu(c["mask"]), cu(c["emb"])
    rc = lib.anyref_op_mask_prompt_embed(None, ptr(mask), ptr(emb), ptr(W["w1"]), ptr(W["b1"]), ptr(W["g1"]), ptr(W["be1"]),
                                         ptr(W["w2"]), ptr(W["b2"]), ptr(W["g2"]), ptr(W["be2"]), ptr(W["w3"]), ptr(W["b3"]),
                                         n, g, C_, c1, c2, ptr(out), max_wg)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", PR.EMBED_CASES, ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_mask_prompt_embed(lib, case):
    n, g, C_, c1, c2, max_wg = case
    c = PR.embed_case(*case)
    rows = n * g * g
    what = f"mask_prompt_embed {case}"
    outs = []
    for cap in sorted({0, max_wg}):
        out = R.nan_fill((rows + GUARD, C_), device="cuda")
        ok(lib, run_embed(lib, c, n, g, C_, c1, c2, out, max_wg=cap))
        R.check_bound(out[:rows].reshape(c["ref"].shape), c["ref"].cuda(), c["bound"].cuda(), c["mutants"], what)
        guards_intact(out, rows, what)
        outs.append(out)
    again = R.nan_fill((rows + GUARD, C_), device="cuda")
    ok(lib, run_embed(lib, c, n, g, C_, c1, c2, again))
    for o in outs:
        assert torch.equal(R.bits(again), R.bits(o)), f"{what}: a rerun or the capped grid gives other bits"


def test_mask_prompt_embed_refusals(lib):
    n, g, C_, c1, c2 = 1, 2, 8, 2, 4
    c = PR.embed_case(n, g, C_, c1, c2)
    out = R.nan_fill((n * g * g + GUARD, 1032), device="cuda")
    # the operands are large enough for none of these; the launcher must refuse before it launches
    for over in (dict(c1=9), dict(c2=33), dict(C_=6), dict(C_=1028), dict(n=0), dict(g=0)):
        a = dict(n=n, g=g, C_=C_, c1=c1, c2=c2)
        a.update(over)
        rc = run_embed(lib, c, a["n"], a["g"], a["C_"], a["c1"], a["c2"], out)
        assert rc != 0 and lib.anyref_op_last_error().decode(), f"accepted {over}"
        assert untouched(out), f"a refused call ({over}) wrote to its output"


# ---- the decoder's f32 attention at the prompted token counts --------------------------------------------------------
@pytest.mark.parametrize("B,H,Sq,Sk,hd", PR.ATTN_CASES)
def test_decoder_attention_forms(lib, B, H, Sq, Sk, hd):
    """launch_attention<float> as Model::mask_decoder calls it with NQ = 10 tokens (4 + 1 output tokens, 2 points, 2 corners,
    text): self attention 10 x 10 at head dim 32, token-to-image 10 x 196 and image-to-token 196 x 10 at head dim 16"""
    g = R._gen(B, H, Sq, Sk, hd, 47)
    q, k, v = (torch.randn(B, S, H, hd, generator=g) for S in (Sq, Sk, Sk))
    scale = 1.0 / hd ** 0.5
    ref, bound = G.attention_form(0, q, k, v, scale)
    out = R.nan_fill((B * Sq + GUARD, H * hd), device="cuda")
    dq, dk, dv = cu(q), cu(k), cu(v)
    rc = lib.anyref_op_attention(0, None, ptr(dq), ptr(dk), ptr(dv), ptr(out), B, H, Sq, Sk, hd, scale, 0, None, None, None, 0, 0)
    ok(lib, rc)
    mut = G.attention_form(0, q, k[:, :-1], v[:, :-1], scale)[0]           # the last key left out
    R.check_bound(out[: B * Sq].reshape(ref.shape), ref.cuda(), bound.cuda(), {"last_key_dropped": mut},
                  f"decoder attention f32 {B}x{H} Sq={Sq} Sk={Sk} hd={hd}")
    guards_intact(out, B * Sq, "decoder attention")
