"""Kernel-level tests of the skinny f32 GEMV (launch_gemv_skinny_f32: every mask-decoder token GEMM and both
text_hidden_fcs layers) and of the glue kernels that only the model's own call paths reach: the mask-decoder tails, the LLM
input assembly, the tower front ends.  References, bounds, mutants and the shapes: tests/glue_ops_ref.py (proved on the CPU by
tests/test_cpu_glue_ops_ref.py, whose ledger also says which test file reaches which launcher).

Every output lives inside a larger buffer prefilled with a fixed NaN bit pattern -- a padded leading dimension where the
kernel has one, guard rows behind every output -- and the guard words are compared as integers afterwards, so a stray write
fails; every element of every output is compared, none is left out.  The only negative cases are shapes a launcher refuses
before it launches."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 2      # guard rows behind every output


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_LIVE = []      # device copies made by cu(): kept until the test ends, so that a pointer handed to the library stays valid


@pytest.fixture(autouse=True)
def _release():
    yield
    _LIVE.clear()


def cu(t, dtype=None):
    if t is None:
        return None
    _LIVE.append(t.to(device="cuda", dtype=dtype or t.dtype).contiguous())
    return _LIVE[-1]


def ok(lib, rc):
    assert rc == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()


def refused(lib, rc, *untouched):
    torch.cuda.synchronize()
    assert rc != 0 and lib.anyref_op_last_error().decode(), "the launcher accepted a shape it must refuse"
    for buf in untouched:
        assert (R.bits(buf) == R.bits(R.nan_fill(buf.shape, buf.dtype, "cuda"))).all(), "a refused call wrote to its output"


def guarded(rows, cols, ld=None, dtype=torch.float32):
    """[rows + GUARD, ld] of the NaN pattern; the kernel's output is [:rows, :cols]"""
    return R.nan_fill((rows + GUARD, ld or cols), dtype, "cuda")


def guards_intact(buf, rows, cols, what):
    """every word outside [:rows, :cols] still holds the pattern"""
    got, pat = R.bits(buf).clone(), R.bits(R.nan_fill(buf.shape, buf.dtype, "cuda")).clone()
    got[:rows, :cols] = 0
    pat[:rows, :cols] = 0
    n = int((got != pat).sum())
    assert n == 0, f"{what}: {n} guard words were written"


def exact(buf, rows, cols, ref, mutants, what):
    """the exact kernels: [:rows, :cols] of buf equals ref (f32 values, converted to buf's dtype without loss) bit for bit"""
    ref = ref.reshape(rows, cols).to(buf.dtype)
    muts = {k: m.reshape(rows, cols) for k, m in mutants.items()}
    R.check_exact(buf[:rows, :cols].contiguous(), ref.cuda(), muts, what)
    guards_intact(buf, rows, cols, what)


# ---- gemv_skinny -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GEMV_CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_gemv_skinny(lib, case):
    B, N, K, ldx, act, resid, ldy, _ = case
    c = R.gemv_case(*case)
    x, W, bias = cu(c["xbuf"]), cu(c["W"]), cu(c["bias"])
    y = guarded(B, N, ldy)
    r = None
    if resid == "alias":
        y[:B, :N] = c["resid"].cuda()
        r = y
    elif resid == "own":
        r = R.nan_fill((B, ldy), device="cuda")        # the residual is read at y's row stride
        r[:, :N] = c["resid"].cuda()
    ok(lib, lib.anyref_op_gemv_skinny(None, ptr(x), ldx, ptr(W), ptr(bias), ptr(y), ldy, ptr(r), B, N, K, act))
    what = f"gemv_skinny {B}x{N}x{K} ldx={ldx} ldy={ldy} act={act} resid={resid}"
    R.check_bound(y[:B, :N], c["ref"].cuda(), c["bound"].cuda(), c["mutants"], what)
    guards_intact(y, B, N, what)


@pytest.mark.parametrize("B,N,K,ldx", R.GEMV_REFUSED)
def test_gemv_skinny_refusals(lib, B, N, K, ldx):
    x = torch.zeros(B * ldx + 8, device="cuda")
    W = torch.zeros(N, K, device="cuda")
    y = guarded(B, N, N + 3)
    refused(lib, lib.anyref_op_gemv_skinny(None, ptr(x), ldx, ptr(W), None, ptr(y), N + 3, None, B, N, K, 0), y)


# ---- mask-decoder tails ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,g,C", R.UPSCALE1_CASES)
def test_upscale1(lib, n, g, C):
    c = R.upscale1_case(n, g, C)
    rows = n * 4 * g * g
    out = guarded(rows, C)
    ok(lib, lib.anyref_op_upscale1(0, None, ptr(cu(c["tmp"])), n, g, C, ptr(cu(c["gain"])), ptr(cu(c["bias"])), R.UPSCALE1_EPS,
                                   ptr(out)))
    what = f"upscale1 n={n} g={g} C={C}"
    R.check_bound(out[:rows], c["ref"].cuda(), c["bound"].cuda(), c["mutants"], what)
    guards_intact(out, rows, C, what)


def test_upscale1_refusals(lib):
    z, out = torch.zeros(4 * 129, device="cuda"), guarded(4, 129)
    refused(lib, lib.anyref_op_upscale1(0, None, ptr(z), 1, 1, 129, ptr(z), ptr(z), 1e-6, ptr(out)), out)
    refused(lib, lib.anyref_op_upscale1(1, None, ptr(z), 1, 1, 64, ptr(z), ptr(z), 1e-6, ptr(out)), out)


@pytest.mark.parametrize("n,ntok,g2,C", R.UPSCALE2_CASES)
def test_upscale2_masks(lib, n, ntok, g2, C):
    c = R.upscale2_case(n, ntok, g2, C)
    px = 4 * g2 * g2
    out = guarded(n * ntok, px)
    ok(lib, lib.anyref_op_upscale2_masks(None, ptr(cu(c["tmp"])), ptr(cu(c["hyper"])), n, ntok, g2, C, ptr(out)))
    what = f"upscale2_masks n={n} ntok={ntok} g2={g2} C={C}"
    R.check_bound(out[:n * ntok], c["ref"].reshape(n * ntok, px).cuda(), c["bound"].reshape(n * ntok, px).cuda(),
                  {k: m.reshape(n * ntok, px) for k, m in c["mutants"].items()}, what)
    guards_intact(out, n * ntok, px, what)


def test_upscale2_masks_refusal(lib):
    z, out = torch.zeros(9 * 4 * 8, device="cuda"), guarded(9, 4)
    refused(lib, lib.anyref_op_upscale2_masks(None, ptr(z), ptr(z), 1, 9, 1, 8, ptr(out)), out)


@pytest.mark.parametrize("g,F", R.DENSE_PE_CASES)
def test_dense_pe(lib, g, F):
    c = R.dense_pe_case(g, F)
    out = guarded(g * g, 2 * F)
    ok(lib, lib.anyref_op_dense_pe(None, ptr(cu(c["gauss"])), g, F, ptr(out)))
    R.check_bound(out[:g * g], c["ref"].cuda(), c["bound"].cuda(), c["mutants"], f"dense_pe g={g} F={F}")
    guards_intact(out, g * g, 2 * F, "dense_pe")


@pytest.mark.parametrize("rows,D", R.L2NORM_CASES)
def test_l2norm_scale(lib, rows, D):
    c = R.l2norm_case(rows, D)
    y = guarded(rows, D)
    ok(lib, lib.anyref_op_l2norm_scale(None, ptr(cu(c["x"])), rows, D, R.L2NORM_SCALE, ptr(y)))
    R.check_bound(y[:rows], c["ref"].cuda(), c["bound"].cuda(), c["mutants"], f"l2norm_scale {rows}x{D}")
    assert (R.bits(y[0]) == 0).all(), "a zero row gives exact (positive) zeros"
    guards_intact(y, rows, D, "l2norm_scale")


@pytest.mark.parametrize("D,n", R.ROWS_CASES)
def test_build_tokens(lib, D, n):
    c = R.rows_case(D, n)
    n_out = c["out_tokens"].shape[0]
    out = guarded(n * (n_out + 1), D)
    ok(lib, lib.anyref_op_build_tokens(None, ptr(cu(c["out_tokens"])), n_out, ptr(cu(c["pred"])), n, D, ptr(out)))
    exact(out, n * (n_out + 1), D, R.build_tokens(c["out_tokens"], c["pred"]), {}, f"build_tokens n={n} C={D}")


@pytest.mark.parametrize("M,D,bmod", R.ADD_ROWS_CASES)
def test_add_rows_and_vec(lib, M, D, bmod):
    c = R.add_rows_case(M, D, bmod)
    a, b, v = cu(c["a"]), cu(c["b"]), cu(c["v"])
    out = guarded(M, D)
    ok(lib, lib.anyref_op_add_rows(None, ptr(a), ptr(b), bmod, ptr(out), M, D))
    exact(out, M, D, c["ref"], c["mutants"], f"add_rows {M}x{D} bmod={bmod}")
    out = guarded(M, D)
    ok(lib, lib.anyref_op_add_vec(None, ptr(a), ptr(v), ptr(out), M, D))
    exact(out, M, D, c["ref_vec"], {}, f"add_vec {M}x{D}")


# ---- LLM input assembly ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt,Smax", R.SPLICE_CASES)
def test_embed_splice(lib, D, dt, Smax):
    c = R.splice_case(D, dt, Smax)
    B, Lmax, n_img, vocab = R.SPLICE_B, R.SPLICE_LMAX, R.SPLICE_NIMG, R.SPLICE_VOCAB
    x = guarded(B * Smax, D)
    out_len = torch.full((B + GUARD,), -7, dtype=torch.int32, device="cuda")
    ok(lib, lib.anyref_op_embed_splice(None, ptr(cu(c["ids"])), ptr(cu(c["lens"])), B, Lmax, ptr(cu(c["table"])), dt, vocab,
                                       ptr(cu(c["img"])), n_img, ptr(x), Smax, D, ptr(out_len)))
    # (rows >= out_len[b] must keep the pattern: they are part of the reference)
    exact(x, B * Smax, D, c["ref"], c["mutants"], f"embed_splice D={D} table={dt} Smax={Smax}")
    assert out_len.tolist() == c["out_len"].tolist() + [-7] * GUARD


@pytest.mark.parametrize("D,n", R.ROWS_CASES)
def test_scatter_gather_rows(lib, D, n):
    c = R.rows_case(D, n)
    Bx, Smax = c["x"].shape[:2]
    out = guarded(n, D)
    ok(lib, lib.anyref_op_gather_rows(None, ptr(cu(c["x"])), Smax, D, ptr(cu(c["gb"])), ptr(cu(c["gp"])), n, ptr(out)))
    exact(out, n, D, R.gather_rows(c["x"], c["gb"], c["gp"]), {}, f"gather_rows n={n} D={D}")
    x = guarded(Bx * Smax, D)
    x0 = R.nan_fill((Bx, Smax, D))
    ok(lib, lib.anyref_op_scatter_rows(None, ptr(cu(c["rows"])), ptr(cu(c["sb"])), ptr(cu(c["sp"])), n, ptr(x), Smax, D))
    exact(x, Bx * Smax, D, R.scatter_rows(c["rows"], c["sb"], c["sp"], x0), {}, f"scatter_rows n={n} D={D}")


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("D,n", R.ROWS_CASES)
def test_embed_rows(lib, D, n, dt):
    c = R.rows_case(D, n)
    table = c["table"].to(R.TABLE_DT[dt])
    out = guarded(n, D)
    ok(lib, lib.anyref_op_embed_rows(None, ptr(cu(c["ids"])), n, ptr(cu(table)), dt, D, ptr(out)))
    exact(out, n, D, R.embed_rows(c["ids"], table), {}, f"embed_rows n={n} D={D} table={dt}")


# ---- tower front ends ------------------------------------------------------------------------------------------------
def roundtrip(lib, ty, m):
    """anyref_op_split_roundtrip of an f32 matrix: the statement of what a pair-typed matrix holds"""
    src, out = cu(m.float()), torch.empty(m.shape, dtype=torch.float32, device="cuda")
    ok(lib, lib.anyref_op_split_roundtrip(ty, None, ptr(src), ptr(out), None, m.shape[0], m.shape[1]))
    return out.cpu()


@pytest.mark.parametrize("B,S,p,Kp,ty", R.flat(R.PATCH_CASES))
def test_im2col_patch(lib, B, S, p, Kp, ty):
    c = R.patch_case(B, S, p, Kp, ty)
    rows = B * (S // p) ** 2
    out = guarded(rows, Kp, dtype=R.sdtype(ty))
    ok(lib, lib.anyref_op_im2col_patch(ty, None, ptr(cu(c["img"])), B, S, p, ptr(out), Kp))
    what = f"im2col_patch t={ty} B={B} S={S} p={p} Kp={Kp}"
    exact(out, rows, Kp, c["ref"], c["mutants"], what)
    if ty in (3, 4):      # bit-identical to the round trip of the f32 matrix
        R.check_exact(out[:rows].cpu(), roundtrip(lib, ty, R.im2col_patch(c["img"], p, Kp, 0)), {}, what + " vs split_roundtrip")


@pytest.mark.parametrize("B,g,C,ty", R.flat(R.C3X3_CASES))
def test_im2col_3x3(lib, B, g, C, ty):
    c = R.c3x3_case(B, g, C, ty)
    rows = B * g * g
    xin = cu(c["x"].reshape(rows, C), R.sdtype(ty))            # t = 3 / 4: f32, split into pairs by the entry point
    out = guarded(rows, 9 * C, dtype=R.sdtype(ty))
    ok(lib, lib.anyref_op_im2col_3x3(ty, None, ptr(xin), B, g, C, ptr(out)))
    what = f"im2col_3x3 t={ty} B={B} g={g} C={C}"
    exact(out, rows, 9 * C, c["ref"], c["mutants"], what)
    if ty in (3, 4):      # the 3 x 3 gather of the round-tripped input
        rt = roundtrip(lib, ty, c["x"].reshape(rows, C)).reshape(B, g, g, C)
        R.check_exact(out[:rows].cpu(), R.im2col_3x3(rt, 0), {}, what + " vs split_roundtrip")


@pytest.mark.parametrize("n,Hh,Ww,k,st,ty", R.flat(R.CONV1_CASES))
def test_im2col_conv1(lib, n, Hh, Ww, k, st, ty):
    c = R.conv1_case(n, Hh, Ww, k, st, ty)
    rows = n * ((Hh - k) // st + 1) * ((Ww - k) // st + 1)
    out = guarded(rows, k * k, dtype=R.sdtype(ty))
    ok(lib, lib.anyref_op_im2col_conv1(ty, None, ptr(cu(c["img"])), n, Hh, Ww, k, st, ptr(out)))
    what = f"im2col_conv1 t={ty} n={n} {Hh}x{Ww} k={k} st={st}"
    exact(out, rows, k * k, c["ref"], c["mutants"], what)
    if ty in (3, 4):
        R.check_exact(out[:rows].cpu(), roundtrip(lib, ty, R.im2col_conv1(c["img"], k, st, 0)), {}, what + " vs split_roundtrip")


@pytest.mark.parametrize("B,n,D,rows", R.CLIP_CASES)
def test_clip_assemble(lib, B, n, D, rows):
    c = R.clip_case(B, n, D, rows)
    Rr = rows if rows > 0 else n + 1
    x = guarded(B * Rr, D)
    ok(lib, lib.anyref_op_clip_assemble(None, ptr(cu(c["patch"])), ptr(cu(c["cls"])), ptr(cu(c["pos"])), ptr(x), B, n, D, rows))
    exact(x, B * Rr, D, c["ref"], c["mutants"], f"clip_assemble B={B} n={n} D={D} rows={rows}")


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_to_f32(lib, dt):
    n = 1000
    src = (torch.randn(n, generator=torch.Generator().manual_seed(dt)) * 50).to(R.TABLE_DT[dt])
    out = guarded(1, n)
    ok(lib, lib.anyref_op_to_f32(None, ptr(cu(src)), dt, ptr(out), n))
    exact(out, 1, n, R.to_f32(src), {}, f"to_f32 dtype={dt}")


@pytest.mark.parametrize("N,K", R.DEQUANT_CASES)
def test_dequant_fp8(lib, N, K):
    c = R.dequant_case(N, K)
    ldq, ldo = K + 16, K + 8
    q = torch.full((N, ldq), 0x7F, dtype=torch.uint8, device="cuda")       # pad bytes: the NaN code
    q[:, :K] = c["q"].cuda()
    out = guarded(N, K, ldo, dtype=torch.bfloat16)
    ok(lib, lib.anyref_op_dequant_fp8(None, ptr(q), ldq, ptr(cu(c["scale"])), N, K, ptr(out), ldo))
    exact(out, N, K, c["ref"], {}, f"dequant_fp8 {N}x{K} ldq={ldq} ldo={ldo}")
