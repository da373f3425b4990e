"""Proves tests/glue_ops_ref.py without a GPU, at the very shapes tests/test_gpu_glue_ops.py runs: for every bounded kernel
an f32 emulation in the kernel's own order (lane chains, butterfly, wave-pair merge ...) lies inside the bound and every mutant
lies outside; for every exact kernel the emulation, which walks the kernel's flat index, equals the reference bit for bit and
every mutant differs.  And the ledger: every launch_* that kernels.h declares is mapped to the op test that reaches it, or
to a model-level test with the reason -- a new launcher cannot land without someone deciding how it is tested."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ops_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- bounded kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GEMV_CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_gemv_skinny(case):
    B, N, K, ldx, act = case[:5]
    c = R.gemv_case(*case)
    emu = R.gemv_skinny(c["xbuf"], ldx, c["W"], c["bias"], c["resid"], act, B, emulate=True)
    R.check_bound(emu, c["ref"], c["bound"], c["mutants"], f"cpu gemv_skinny {B}x{N}x{K} ldx={ldx} act={act}")


def test_gemv_skinny_mutants_cover_every_loss():
    """every loss of gemv_skinny is exercised by at least one case (each needs a shape that can show it)"""
    seen = set()
    for case in R.GEMV_CASES:
        B, N, K, ldx, act, resid = case[:6]
        seen |= {"drop4"} | ({"odd_wave"} if K > R.GEMV_CH else set()) | ({"act_after_resid"} if act and resid else set()) | \
            ({"resid_row0"} if B >= 2 and resid else set()) | ({"ldx_ignored"} if B >= 2 and ldx != K else set())
    assert seen == {"drop4", "odd_wave", "act_after_resid", "resid_row0", "ldx_ignored"}


@pytest.mark.parametrize("n,g,C", R.UPSCALE1_CASES)
def test_upscale1(n, g, C):
    c = R.upscale1_case(n, g, C)
    emu = R.upscale1(c["tmp"], n, g, C, c["gain"], c["bias"], R.UPSCALE1_EPS, emulate=True)
    R.check_bound(emu, c["ref"], c["bound"], c["mutants"], f"cpu upscale1 n={n} g={g} C={C}")


@pytest.mark.parametrize("n,ntok,g2,C", R.UPSCALE2_CASES)
def test_upscale2_masks(n, ntok, g2, C):
    c = R.upscale2_case(n, ntok, g2, C)
    emu = R.upscale2_masks(c["tmp"], c["hyper"], n, ntok, g2, C, emulate=True)
    R.check_bound(emu, c["ref"], c["bound"], c["mutants"], f"cpu upscale2 n={n} ntok={ntok} g2={g2} C={C}")


@pytest.mark.parametrize("g,F", R.DENSE_PE_CASES)
def test_dense_pe(g, F):
    c = R.dense_pe_case(g, F)
    R.check_bound(R.dense_pe(c["gauss"], g, F, emulate=True), c["ref"], c["bound"], c["mutants"], f"cpu dense_pe g={g} F={F}")


@pytest.mark.parametrize("rows,D", R.L2NORM_CASES)
def test_l2norm_scale(rows, D):
    c = R.l2norm_case(rows, D)
    emu = R.l2norm_scale(c["x"], R.L2NORM_SCALE, emulate=True)
    R.check_bound(emu, c["ref"], c["bound"], c["mutants"], f"cpu l2norm_scale {rows}x{D}")
    assert (R.bits(emu[0]) == 0).all() and (c["ref"][0] == 0).all() and (c["bound"][0] == 0).all(), "a zero row gives exact zeros"


# ---- exact kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,p,Kp,ty", R.flat(R.PATCH_CASES))
def test_im2col_patch(B, S, p, Kp, ty):
    c = R.patch_case(B, S, p, Kp, ty)
    R.check_exact(R.im2col_patch(c["img"], p, Kp, ty, emulate=True), c["ref"], c["mutants"], f"cpu im2col_patch t={ty} {B},{S},{p},{Kp}")


@pytest.mark.parametrize("B,g,C,ty", R.flat(R.C3X3_CASES))
def test_im2col_3x3(B, g, C, ty):
    c = R.c3x3_case(B, g, C, ty)
    R.check_exact(R.im2col_3x3(c["x"], ty, emulate=True), c["ref"], c["mutants"], f"cpu im2col_3x3 t={ty} {B},{g},{C}")


@pytest.mark.parametrize("n,Hh,Ww,k,st,ty", R.flat(R.CONV1_CASES))
def test_im2col_conv1(n, Hh, Ww, k, st, ty):
    c = R.conv1_case(n, Hh, Ww, k, st, ty)
    R.check_exact(R.im2col_conv1(c["img"], k, st, ty, emulate=True), c["ref"], c["mutants"], f"cpu im2col_conv1 t={ty} {n},{Hh},{Ww},{k},{st}")


def test_exact_mutants_cover_every_loss():
    """the shape-dependent mutants of the exact kernels each appear in at least one case"""
    assert any(Kp > 3 * p * p for _, _, p, Kp, _ in R.PATCH_CASES) and any(g > 1 for _, g, _, _ in R.C3X3_CASES)
    assert any(rows > n + 1 for _, n, _, rows in R.CLIP_CASES) and any(bmod < M for M, _, bmod in R.ADD_ROWS_CASES)


@pytest.mark.parametrize("D,dt,Smax", R.SPLICE_CASES)
def test_embed_splice(D, dt, Smax):
    c = R.splice_case(D, dt, Smax)
    emu, emu_len = R.embed_splice(c["ids"], c["lens"], c["table"], R.SPLICE_VOCAB, c["img"], c["x0"], emulate=True)
    R.check_exact(emu, c["ref"], c["mutants"], f"cpu embed_splice D={D} table={dt} Smax={Smax}")
    assert emu_len.tolist() == c["out_len"].tolist() == [16, 7, 7, 12]
    assert int(c["out_len"].max()) <= Smax
    # what the case is there to show: sentinel rows past out_len, zero rows for the foreign ids, image rows, widened table rows
    ref = c["ref"]
    assert (R.bits(ref[1, 7:]) == R.NAN_BITS).all() and (ref[0, 13] == 0).all() and (ref[2, 5:7] == 0).all()
    assert torch.equal(ref[3, 7:12], c["img"][3]) and torch.equal(ref[0, 0], c["table"][c["ids"][0, 0]].float())


@pytest.mark.parametrize("D,n", R.ROWS_CASES)
def test_row_copies(D, n):
    c = R.rows_case(D, n)
    R.check_exact(R.gather_rows(c["x"], c["gb"], c["gp"], emulate=True), R.gather_rows(c["x"], c["gb"], c["gp"]), {}, "cpu gather_rows")
    x0 = R.nan_fill(c["x"].shape)
    R.check_exact(R.scatter_rows(c["rows"], c["sb"], c["sp"], x0, emulate=True), R.scatter_rows(c["rows"], c["sb"], c["sp"], x0), {},
                  "cpu scatter_rows")
    assert len({(int(b), int(p)) for b, p in zip(c["sb"], c["sp"])}) == n, "scatter destinations are distinct"
    R.check_exact(R.build_tokens(c["out_tokens"], c["pred"], emulate=True), R.build_tokens(c["out_tokens"], c["pred"]), {},
                  "cpu build_tokens")


@pytest.mark.parametrize("B,n,D,rows", R.CLIP_CASES)
def test_clip_assemble(B, n, D, rows):
    c = R.clip_case(B, n, D, rows)
    emu = R.clip_assemble(c["patch"], c["cls"], c["pos"], rows, c["x0"], emulate=True)
    R.check_exact(emu, c["ref"], c["mutants"], f"cpu clip_assemble {B},{n},{D},{rows}")


@pytest.mark.parametrize("M,D,bmod", R.ADD_ROWS_CASES)
def test_add_rows_and_vec(M, D, bmod):
    c = R.add_rows_case(M, D, bmod)
    R.check_exact(R.add_rows(c["a"], c["b"], bmod, emulate=True), c["ref"], c["mutants"], f"cpu add_rows {M},{D},{bmod}")
    R.check_exact(R.add_vec(c["a"], c["v"], emulate=True), c["ref_vec"], {}, f"cpu add_vec {M},{D}")


@pytest.mark.parametrize("N,K", R.DEQUANT_CASES)
def test_dequant_fp8(N, K):
    c = R.dequant_case(N, K)
    R.check_exact(R.dequant_fp8_emulate(c["q"], c["scale"]), c["ref"], {}, f"cpu dequant_fp8 {N}x{K}")


# ---- the ledger ------------------------------------------------------------------------------------------------------
_G = "tests/test_gpu_glue_ops.py"
_O = "tests/test_gpu_ops.py"
# launcher -> ("op", anyref_op_* symbol, test file that calls it)  |  ("via", test file, why no op test of its own)
LEDGER = {
    "launch_gemm": ("op", "anyref_op_gemm", _O),
    "launch_gemv": ("op", "anyref_op_gemv", _O),
    "launch_gemv_skinny_f32": ("op", "anyref_op_gemv_skinny", _G),
    "launch_quant_fp8_rows": ("op", "anyref_op_quant_fp8", "tests/test_gpu_fp8w.py"),
    "launch_dequant_fp8_rows": ("op", "anyref_op_dequant_fp8", _G),
    "launch_quant_int4_rows": ("op", "anyref_op_quant_int4", "tests/test_gpu_int4w.py"),
    "launch_dequant_int4_rows": ("op", "anyref_op_dequant_int4", "tests/test_gpu_int4w.py"),
    "launch_lora_merge": ("op", "anyref_op_lora_merge", "tests/test_gpu_adapter_ops.py"),
    "launch_gemv_int4": ("op", "anyref_op_gemv_int4", "tests/test_gpu_int4w.py"),
    "launch_norm": ("op", "anyref_op_norm", _O),
    "launch_attention": ("op", "anyref_op_attention", _O),
    "launch_decode_attn": ("op", "anyref_op_decode_attn", "tests/test_gpu_decode_ops.py"),
    "launch_decode_step_attn": ("op", "anyref_op_decode_attn", "tests/test_gpu_decode_ops.py"),
    "launch_attn_row_mean": ("via", "tests/test_gpu_rephrase_paths.py",
                             "the per-image rephrase chain; the model runs it with the fused paths off and is compared with them on"),
    "launch_rel_pos": ("op", "anyref_op_rel_pos", _O),
    "launch_im2col_patch": ("op", "anyref_op_im2col_patch", _G),
    "launch_im2col_3x3": ("op", "anyref_op_im2col_3x3", _G),
    "launch_convert": ("op", "anyref_op_split_roundtrip", "tests/test_gpu_parity16_f16_ops.py"),
    "launch_unsplit": ("op", "anyref_op_split_roundtrip", "tests/test_gpu_parity16_f16_ops.py"),
    "launch_add_rows": ("op", "anyref_op_add_rows", _G),
    "launch_clip_assemble": ("op", "anyref_op_clip_assemble", _G),
    "launch_im2col_conv1": ("op", "anyref_op_im2col_conv1", _G),
    "launch_l2norm_scale": ("op", "anyref_op_l2norm_scale", _G),
    "launch_embed_splice": ("op", "anyref_op_embed_splice", _G),
    "launch_scatter_rows": ("op", "anyref_op_scatter_rows", _G),
    "launch_rope_cache_slabs": ("op", "anyref_op_rope_cache", "tests/test_gpu_gemm_forms.py"),
    "launch_rope_cache": ("op", "anyref_op_rope_cache", "tests/test_gpu_decode_ops.py"),
    "launch_rope_cache_f32": ("op", "anyref_op_decode_attn", "tests/test_gpu_decode_ops.py"),
    "launch_embed_rows": ("op", "anyref_op_embed_rows", _G),
    "launch_kv_broadcast": ("op", "anyref_op_kv_broadcast", "tests/test_gpu_session_ops.py"),
    "launch_kv_gather": ("op", "anyref_op_kv_gather", "tests/test_gpu_session_pool_ops.py"),
    "launch_build_tokens": ("op", "anyref_op_build_tokens", _G),
    "launch_argmax": ("op", "anyref_op_argmax", "tests/test_gpu_decode_ops.py"),
    "launch_argmax_next": ("op", "anyref_op_argmax", "tests/test_gpu_decode_ops.py"),
    "launch_token_scores": ("op", "anyref_op_token_scores", "tests/test_gpu_token_scores_ops.py"),
    "launch_draft_accept": ("op", "anyref_op_draft_accept", "tests/test_gpu_draft_ops.py"),
    "launch_upscale1": ("op", "anyref_op_upscale1", _G),
    "launch_upscale2_masks": ("op", "anyref_op_upscale2_masks", _G),
    "launch_postprocess": ("op", "anyref_op_postprocess", _O),
    "launch_dense_pe": ("op", "anyref_op_dense_pe", _G),
    "launch_fill_rows_bias": ("op", "anyref_op_norm_ex", "tests/test_gpu_gemm_forms.py"),
    "launch_iou_counts": ("via", "tests/test_gpu_evalops.py", "anyref_amd.evalops wraps anyref_op_iou_counts; checked against the reference formula there"),
    "launch_avs_counts": ("via", "tests/test_gpu_evalops.py", "anyref_amd.evalops wraps anyref_op_avs_counts; checked against the threshold sweep there"),
    "launch_pool_ref_tokens": ("op", "anyref_op_pool_ref_tokens", "tests/test_gpu_refimg.py"),
    "launch_pil_resample_u8": ("via", "tests/test_gpu_preprocess.py", "anyref_amd.preprocess wraps anyref_op_pil_resample_u8; bit-exact against Pillow fixtures there"),
    "launch_clip_finish": ("via", "tests/test_gpu_preprocess.py", "anyref_amd.preprocess wraps anyref_op_clip_finish; against the HF fixtures there"),
    "launch_kaldi_fbank": ("via", "tests/test_gpu_preprocess.py", "anyref_amd.preprocess wraps anyref_op_kaldi_fbank; against the oracle's filterbank there"),
    "launch_sam_preprocess": ("via", "tests/test_gpu_evalops.py", "anyref_amd.evalops wraps anyref_op_sam_preprocess; bit-exact there"),
    "launch_add_vec": ("op", "anyref_op_add_vec", _G),
    "launch_gather_rows": ("op", "anyref_op_gather_rows", _G),
    "launch_rephrase": ("via", "tests/test_gpu_rephrase_paths.py",
                        "the per-image rephrase chain; the model runs it with the fused paths off and is compared with them on"),
    "launch_seg_attn_span": ("op", "anyref_op_seg_rephrase", "tests/test_gpu_rephrase_ops.py"),
    "launch_seg_rephrase_apply": ("op", "anyref_op_seg_rephrase", "tests/test_gpu_rephrase_ops.py"),
    "launch_seg_rephrase": ("op", "anyref_op_seg_rephrase", "tests/test_gpu_rephrase_ops.py"),
    "launch_to_f32": ("op", "anyref_op_to_f32", _G),
}


def _read(rel):
    with open(os.path.join(ROOT, rel)) as f:
        return f.read()


def declared_launchers(text):
    """every launch_* a header declares: the names in front of an argument list, comments left out"""
    code = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", text), flags=re.S)
    return set(re.findall(r"\b(launch_\w+)\s*\(", code))


def ledger_problems(ledger, declared):
    from anyref_amd import _lib
    header = _read("include/anyref_hip_ops.h")
    out = [f"{n}: declared in kernels.h, no line in the ledger" for n in sorted(declared - set(ledger))]
    out += [f"{n}: in the ledger, no longer declared in kernels.h" for n in sorted(set(ledger) - declared)]
    for name, entry in sorted(ledger.items()):
        if entry[0] == "op":
            _, sym, path = entry
            if sym not in _lib.SYMBOLS:
                out.append(f"{name}: {sym} is not in _lib.SYMBOLS")
            if not re.search(r"\b%s\s*\(" % re.escape(sym), header):
                out.append(f"{name}: {sym} is not declared in include/anyref_hip_ops.h")
            if not os.path.exists(os.path.join(ROOT, path)) or not re.search(r"\b%s\b" % re.escape(sym), _read(path)):
                out.append(f"{name}: {path} does not call {sym}")
        elif entry[0] == "via":
            _, path, why = entry
            if not os.path.exists(os.path.join(ROOT, path)) or not os.path.basename(path).startswith("test_"):
                out.append(f"{name}: {path} is not a test file")
            if len(why.split()) < 4:
                out.append(f"{name}: a 'via' line needs its reason")
        else:
            out.append(f"{name}: unknown kind {entry[0]!r}")
    return out


def test_ledger_every_launcher_has_a_test():
    declared = declared_launchers(_read("anyref_amd/csrc/kernels.h"))
    assert len(declared) > 40, "kernels.h was not parsed"
    problems = ledger_problems(LEDGER, declared)
    assert not problems, "\n".join(problems)


def test_ledger_notices_a_missing_or_stale_line():
    declared = declared_launchers(_read("anyref_amd/csrc/kernels.h"))
    short = {k: v for k, v in LEDGER.items() if k != "launch_dense_pe"}
    assert any("launch_dense_pe" in p for p in ledger_problems(short, declared))
    stale = dict(LEDGER, launch_swiglu=("op", "anyref_op_gemm", _O))
    assert any("launch_swiglu" in p for p in ledger_problems(stale, declared))
    wrong = dict(LEDGER, launch_dense_pe=("op", "anyref_op_dense_pe", _O))
    assert any("does not call" in p for p in ledger_problems(wrong, declared))
    assert declared_launchers("// launch_ghost(int)\nvoid launch_real(int a);\n/* launch_other( */") == {"launch_real"}
