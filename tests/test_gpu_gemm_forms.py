"""Kernel-level tests of the GEMM, norm and attention launch forms only the model uses (model.hip), through
anyref_op_gemm_ex / anyref_op_norm_ex / anyref_op_attention_ex: split-K with the norm fused in, the SwiGLU pair epilogue,
raw split-K slabs, batched launches with element strides, capped launches (max_wg), padded leading dimensions; the norm's
16-bit outputs, row map, activation and fill side job; attention over a fused qkv buffer and a KV cache with ragged lengths.
References, bounds and mutants: tests/gemm_forms_ref.py (proved on the CPU by tests/test_cpu_gemm_forms_ref.py); every
element is checked, the tag a named form books and the fusion flag are asserted."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_forms_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -768.0      # exact in bf16 and f16
_PRE = {1: "gemm_bf16_", 2: "gemm_f16_", 3: "gemm_sp16_", 4: "gemm_sp16h_"}


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def adt(ty):
    """dtype of an activation at the interface (pairs: f32)"""
    return torch.float32 if ty in (0, 3, 4) else R.wdtype(ty)


def lay(t2d, ld, dtype, fill=0.0):
    """[rows, cols] -> device buffer [rows, ld] of dtype with the values in the leading columns"""
    buf = torch.full((t2d.shape[0], ld), fill, dtype=dtype, device="cuda")
    buf[:, : t2d.shape[1]] = t2d.to(dtype)
    return buf


def ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


def call(lib, fn, ty, e):
    rc = fn(ty, None, C.byref(e))
    assert rc == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()
    return lib.anyref_op_last_tags().decode().split(",")


def gemm_ex(lib, ty, **kw):
    from anyref_amd._lib import GemmEx
    e = GemmEx()
    e.alpha, e.batch = 1.0, 1
    for k, v in kw.items():
        setattr(e, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    tags = call(lib, lib.anyref_op_gemm_ex, ty, e)
    return tags, e.norm_done


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


# ---- split-K reduction with the norm fused in ------------------------------------------------------------------------
# (M, N, K, LayerNorm, tile tag or None).  The launcher has seven splitk_reduce_norm_kernel<threads, slices, columns>
# instantiations (slices 0 = run-time count); each row names the one it reaches:
#   320 x 4096 x 4096, 320 x 4096 x 11008   LLaMA o_proj / down_proj          <1024, 4, 1>
#   257 x 1024 x 4096                        CLIP fc2, 8 slices                <256, 8, 1>
#   257 x 1024 x 1024                        CLIP out_proj, 2 slices           <256, 2, 1>
#   320 x 5120 x 13824                       13B down_proj, 4 slices           <1024, 4, 2>
#   9 x 4096 x 4096                          decode rows, 8 slices             <1024, 0, 1>
#   16 x 4096 x 11008                        decode rows, 4 slices             <1024, 4, 1>
#   257 x 1024 x 3072                        4 slices at N <= 1024             <256, 0, 1>
#   16 x 5120 x 4096                         8 slices at N > 4096              <1024, 0, 2>
#   300 x 4100 x 4096                        ragged neighbour, N % 128 != 0    <1024, 4, 2>
# (16 x 5120 has K = 4096: over 16 rows the bound of 2 x 13824 pair products is too wide to see eight lost columns)
FUSED = [(320, 4096, 4096, False, "320x64"), (320, 4096, 11008, False, "320x64"), (257, 1024, 4096, True, None),
         (257, 1024, 1024, True, None), (320, 5120, 13824, False, None), (9, 4096, 4096, False, "_dec"),
         (16, 4096, 11008, False, "_dec"), (257, 1024, 3072, True, None), (16, 5120, 4096, False, "_dec"),
         (300, 4100, 4096, False, None)]      # ragged neighbour: N % 128 != 0 (N % 4 == 0)


@pytest.mark.parametrize("ty", [1, 2, 3, 4])
@pytest.mark.parametrize("M,N,K,ln,tag", FUSED)
def test_splitk_fused_norm(lib, ty, M, N, K, ln, tag):
    A, W, bias, resid, gain, nbias = cu(*R.gemm_operands(M, N, K, M + N + K, small_rows=True, row_offset=ln, with_bias=ln))
    eps = 1e-6
    ldw, nld = K + 64, N + 64                                  # weight rows padded by 128 bytes, as every LLM weight is
    Ad, Wd = lay(A[0], K, adt(ty)), lay(W[0], ldw, R.wdtype(ty))
    Cd = resid[0].clone().contiguous()                         # the residual stream: resid == C, f32
    nout = torch.full((M, nld), SENT, dtype=adt(ty), device="cuda")
    tags, done = gemm_ex(lib, ty, A=Ad, W=Wd, bias=bias[0] if ln else None, C=Cd, resid=Cd, M=M, N=N, K=K, lda=K, ldw=ldw,
                         ldc=N, ldr=N, c_f32=1, norm_gain=gain, norm_bias=nbias if ln else None, norm_out=nout,
                         norm_ld=nld, norm_eps=eps)
    assert done == 1, f"the norm was not fused (tags {tags})"
    if tag:
        assert any(t.startswith(_PRE[ty]) and tag in t for t in tags), (tag, tags)
    kw = dict(bias=bias if ln else None, resid=resid, c_f32=True, norm={"gain": gain, "bias": nbias if ln else None, "eps": eps})
    out = R.gemm_form(ty, A, W, **kw)
    losses = ["drop_k", "norm_before_resid", "no_eps"] + (["ln_keeps_mean"] if ln else [])
    muts = {n: R.gemm_form(ty, A, W, loss=n, **kw)["norm"][0][0] for n in losses}
    what = f"fused norm t={ty} {M}x{N}x{K} ln={ln} [{'+'.join(tags)}]"
    R.check_bound(nout[:, :N], out["norm"][0][0], out["norm"][1][0], muts, what)
    assert (nout[:, N:] == SENT).all(), "norm_out written past N"
    R.check_bound(Cd, out["C"][0][0], out["C"][1][0], R.gemm_form(ty, A, W, loss="drop_k", **kw)["C"][0][0], what + " C")


@pytest.mark.parametrize("ty", [1, 2])
@pytest.mark.parametrize("M,N,K,ln", [(320, 4096, 1024, False), (64, 8196, 4096, False), (600, 1024, 4096, True)])
def test_norm_not_fused_leaves_norm_out_alone(lib, ty, M, N, K, ln):
    """K < 2048 without norm_bias, N > 8192, M > 512: the launcher does not fuse -- flag clear, norm_out untouched, C right"""
    A, W, bias, resid, gain, nbias = cu(*R.gemm_operands(M, N, K, M + N + K))
    Ad, Wd = lay(A[0], K, adt(ty)), lay(W[0], K, R.wdtype(ty))
    Cd = resid[0].clone().contiguous()
    nout = torch.full((M, N), SENT, dtype=adt(ty), device="cuda")
    tags, done = gemm_ex(lib, ty, A=Ad, W=Wd, C=Cd, resid=Cd, M=M, N=N, K=K, lda=K, ldw=K, ldc=N, ldr=N, c_f32=1,
                         norm_gain=gain, norm_bias=nbias if ln else None, norm_out=nout, norm_ld=N, norm_eps=1e-6)
    assert done == 0 and (nout == SENT).all(), tags
    out = R.gemm_form(ty, A, W, resid=resid)
    R.check_bound(Cd, out["C"][0][0], out["C"][1][0], R.gemm_form(ty, A, W, resid=resid, loss="drop_k")["C"][0][0],
                  f"unfused t={ty} {M}x{N}x{K} [{'+'.join(tags)}]")


# ---- SwiGLU pair epilogue --------------------------------------------------------------------------------------------
SWIGLU = [(320, 22016, 4096, "320x96s3"), (257, 22016, 4096, "320x96s3"), (1280, 22016, 4096, "256x256"),
          (8, 22016, 4096, "_dec"),            # two K slices: splitk_reduce_kernel's pair branch
          (64, 512, 8192, None),               # deep K, eight slices through the same branch
          (100, 1028, 192, None)]              # ragged neighbour on the plain tiles


@pytest.mark.parametrize("ty,c_f32", [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (4, 1)])
@pytest.mark.parametrize("M,N,K,tag", SWIGLU)
def test_swiglu_pairs(lib, ty, c_f32, M, N, K, tag):
    A, W, *_ = cu(*R.gemm_operands(M, N, K, M + N + K, w_scale=0.02))
    ldw, ldc = K + 64, N // 2 + 64
    Ad, Wd = lay(A[0], K, adt(ty)), lay(W[0], ldw, R.wdtype(ty))
    Cd = torch.full((M, ldc), SENT, dtype=torch.float32 if c_f32 else adt(ty), device="cuda")
    tags, _ = gemm_ex(lib, ty, A=Ad, W=Wd, C=Cd, M=M, N=N, K=K, lda=K, ldw=ldw, ldc=ldc, c_f32=c_f32, swiglu_pairs=1)
    if tag:
        assert any(t.startswith(_PRE[ty]) and tag in t for t in tags), (tag, tags)
    kw = dict(swiglu=True, c_f32=bool(c_f32))
    ref, bound = R.gemm_form(ty, A, W, **kw)["C"]
    muts = {n: R.gemm_form(ty, A, W, loss=n, **kw)["C"][0][0] for n in ("drop_k", "swap_gate_up", "not_interleaved")}
    R.check_bound(Cd[:, : N // 2], ref[0], bound[0], muts, f"swiglu t={ty} c_f32={c_f32} {M}x{N}x{K} [{'+'.join(tags)}]")
    assert (Cd[:, N // 2:] == SENT).all(), "C written past N / 2"


# ---- raw split-K slabs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", [1, 2, 3, 4])
@pytest.mark.parametrize("M,N,K,tag", [(320, 12288, 4096, "320x96s3"), (257, 12288, 4096, "320x96s3"), (100, 392, 256, None)])
def test_raw_slabs(lib, ty, M, N, K, tag):
    A, W, *_ = cu(*R.gemm_operands(M, N, K, M + N + K))
    ldw = K + 64
    Ad, Wd = lay(A[0], K, adt(ty)), lay(W[0], ldw, R.wdtype(ty))
    sl = torch.full((2, M, N), SENT, device="cuda")
    tags, _ = gemm_ex(lib, ty, A=Ad, W=Wd, M=M, N=N, K=K, lda=K, ldw=ldw, ldc=N, slabs_out=sl, slabs=2)
    if tag:
        assert any(t.startswith(_PRE[ty]) and tag in t for t in tags), (tag, tags)
    ref, bound = R.gemm_form(ty, A, W, slabs=2)["slabs"]
    muts = {n: R.gemm_form(ty, A, W, slabs=2, loss=n)["slabs"][0] for n in ("drop_k", "slab_swapped", "slab_missing")}
    R.check_bound(sl, ref, bound, muts, f"raw slabs t={ty} {M}x{N}x{K} [{'+'.join(tags)}]")


@pytest.mark.parametrize("ty", [1, 2])
def test_raw_slabs_chained_into_rope_cache(lib, ty):
    """prefill qkv as the model runs it at one sequence of 320: the GEMM writes two K slabs (320 x 12288 x 4096), the RoPE +
    cache kernel sums them, rounds to T, rotates q / k and appends k / v.  Against float64 of the whole chain, and against
    the single-GEMM path (T output, then the plain RoPE kernel) under the same bound."""
    S, H, hd, K, maxS, pos0 = 320, 32, 128, 4096, 640, 100
    N = 3 * H * hd
    A, W, *_ = cu(*R.gemm_operands(S, N, K, 99))
    Ad, Wd = lay(A[0], K, adt(ty)), lay(W[0], K + 64, R.wdtype(ty))
    sl = torch.empty(2, S, N, device="cuda")
    tags, _ = gemm_ex(lib, ty, A=Ad, W=Wd, M=S, N=N, K=K, lda=K, ldw=K + 64, ldc=N, slabs_out=sl, slabs=2)
    assert any("320x96s3" in t for t in tags), tags
    tab = torch.empty(maxS, 2, hd // 2)
    assert lib.anyref_op_rope_table(maxS, hd, 10000.0, C.c_void_p(tab.data_ptr())) == 0
    tab_d = tab.cuda()
    p0 = torch.tensor([pos0], dtype=torch.int32, device="cuda")

    def rope(qkv, s0, s1):
        q_out = torch.full((1, S, H, hd), SENT, dtype=adt(ty), device="cuda")
        kc, vc = (torch.full((1, maxS, H, hd), SENT, dtype=adt(ty), device="cuda") for _ in range(2))
        rc = lib.anyref_op_rope_cache(ty, None, ptr(qkv), ptr(s0), ptr(s1), 1, S, H, hd, ptr(p0), None, ptr(tab_d), ptr(q_out),
                                      ptr(kc), ptr(vc), maxS, None)
        assert rc == 0, lib.anyref_op_last_error().decode()
        torch.cuda.synchronize()
        return {"q": q_out[0], "k": kc[0], "v": vc[0]}
    chained = rope(None, sl[0], sl[1])
    single_c = torch.empty(S, N, dtype=adt(ty), device="cuda")
    gemm_ex(lib, ty, A=Ad, W=Wd, C=single_c, M=S, N=N, K=K, lda=K, ldw=K + 64, ldc=N, c_f32=0)
    single = rope(single_c, None, None)
    cs, sn = tab_d[pos0: pos0 + S, 0], tab_d[pos0: pos0 + S, 1]

    def chain(loss=None):
        ref, bnd = R.gemm_form(ty, A, W, slabs=2, loss=loss)["slabs"]
        return R.rope_chain_form(ty, ref.sum(0).view(S, 3, H, hd), bnd.sum(0).view(S, 3, H, hd), cs, sn)
    out, m1, m2 = chain(), chain("slab_missing"), chain("drop_k")
    for key in ("q", "k", "v"):
        ref, bnd = out[key]
        if key != "q":      # the cache: rows outside [pos0, pos0 + S) keep their sentinel exactly
            full, fb = torch.full((maxS, H, hd), SENT, dtype=torch.float64, device="cuda"), torch.zeros(maxS, H, hd, device="cuda")
            muts = {}
            for name, m in (("slab_missing", m1), ("drop_k", m2)):
                muts[name] = full.clone()
                muts[name][pos0: pos0 + S] = m[key][0]
            muts["pos0_ignored"] = full.clone()
            muts["pos0_ignored"][:S] = ref
            full[pos0: pos0 + S], fb[pos0: pos0 + S] = ref, bnd
            ref, bnd = full, fb
        else:
            muts = {"slab_missing": m1[key][0], "drop_k": m2[key][0]}
        R.check_bound(chained[key], ref, bnd, muts, f"slabs -> rope t={ty} {key} (chained)")
        R.check_bound(single[key], ref, bnd, muts, f"slabs -> rope t={ty} {key} (single GEMM)")


# ---- batched launches with element strides ---------------------------------------------------------------------------
@pytest.mark.parametrize("ty", [1, 2])
@pytest.mark.parametrize("rows", [4096, 4900, 196])
def test_batched_rel_pos_layout(lib, ty, rows):
    """the SAM rel-pos GEMM: batch = 16 heads, A = the q columns of the fused qkv buffer (sA = hd, lda = 3 D), one shared
    table (sW = 0) whose K is padded from 80 to 128 with zero weights (A reads on into the next head there), P f32 [H][rows][n]"""
    H, hd, n, K = 16, 80, 256, 128
    D = H * hd
    g = torch.Generator().manual_seed(rows)
    qkv = torch.randn(rows, 3 * D, generator=g).cuda()
    W = (torch.randn(1, n, K, generator=g) * 0.3).cuda()
    W[..., hd:] = 0
    qd, Wd = qkv.to(adt(ty)), lay(W[0], K, R.wdtype(ty))
    Pd = torch.full((H, rows, n), SENT, device="cuda")
    tags, _ = gemm_ex(lib, ty, A=qd, W=Wd, C=Pd, M=rows, N=n, K=K, lda=3 * D, ldw=K, ldc=n, c_f32=1, batch=H, sA=hd,
                      sW=0, sC=rows * n)
    A = torch.stack([qkv[:, z * hd: z * hd + K] for z in range(H)])
    ref, bound = R.gemm_form(ty, A, W)["C"]
    muts = {k: R.gemm_form(ty, A, W, loss=k, k_real=hd)["C"][0] for k in ("drop_k", "z_on_shared_w")}
    R.check_bound(Pd, ref, bound, muts, f"batched rel-pos t={ty} rows {rows} [{'+'.join(tags)}]")


@pytest.mark.parametrize("ty", [1, 2])
@pytest.mark.parametrize("B", [2, 4])
def test_batched_patch_embedding(lib, ty, B):
    """batch = images, one residual (the position embedding) shared by all: sR = 0"""
    M, N, K = 4096, 1280, 768
    A, W, bias, resid, *_ = cu(*R.gemm_operands(M, N, K, B, Z=B))
    Ad, Wd = A.to(adt(ty)).contiguous(), lay(W[0], K, R.wdtype(ty))
    Cd = torch.full((B, M, N), SENT, device="cuda")
    rd = resid[:1].contiguous()
    tags, _ = gemm_ex(lib, ty, A=Ad, W=Wd, bias=bias[0], C=Cd, resid=rd, M=M, N=N, K=K, lda=K, ldw=K, ldc=N, ldr=N, c_f32=1,
                      batch=B, sA=M * K, sC=M * N, sR=0, max_wg=128)
    kw = dict(bias=bias[:1], resid=rd)
    ref, bound = R.gemm_form(ty, A, W, **kw)["C"]
    muts = {k: R.gemm_form(ty, A, W, loss=k, **kw)["C"][0] for k in ("drop_k", "resid_per_batch")}
    R.check_bound(Cd, ref, bound, muts, f"batched patch embedding t={ty} B={B} [{'+'.join(tags)}]")


@pytest.mark.parametrize("ty", [0, 1, 2])
def test_batched_bias_stride_relu_alpha(lib, ty):
    """the hypernetwork MLPs' form: per-batch W, bias (sBias) and C (sC), ReLU; and alpha != 1"""
    Z, M, N, K = 4, 33, 256, 256
    A, W, bias, *_ = cu(*R.gemm_operands(M, N, K, 77, Z=Z, Zw=Z))
    Ad, Wd = A.to(adt(ty)).contiguous(), W.to(R.wdtype(ty)).contiguous()
    Cd = torch.full((Z, M, N), SENT, dtype=adt(ty), device="cuda")
    tags, _ = gemm_ex(lib, ty, A=Ad, W=Wd, bias=bias.contiguous(), C=Cd, M=M, N=N, K=K, lda=K, ldw=K, ldc=N, c_f32=0, batch=Z,
                      sA=M * K, sW=N * K, sC=M * N, sBias=N, act=R.ACT_RELU, alpha=0.125)
    kw = dict(bias=bias, act=R.ACT_RELU, alpha=0.125, c_f32=False)
    if ty == 0:      # f32 MFMA: products are not exact; the f32 tolerance of test_gpu_ops.test_gemm
        ref = torch.relu(0.125 * A @ W.transpose(1, 2) + bias[:, None])
        tol = 8e-5 * max(1.0, ref.abs().max().item())
        assert (Cd - ref).abs().max().item() <= tol
        for name in ("drop_k", "alpha_ignored"):      # the same losses lie outside that tolerance
            mut = R.gemm_form(1, A, W, loss=name, **kw)["C"][0]
            assert (mut - R.gemm_form(1, A, W, **kw)["C"][0]).abs().max().item() > 100 * tol, name
        return
    ref, bound = R.gemm_form(ty, A, W, **kw)["C"]
    muts = {k: R.gemm_form(ty, A, W, loss=k, **kw)["C"][0] for k in ("drop_k", "alpha_ignored")}
    R.check_bound(Cd, ref, bound, muts, f"batched bias relu alpha t={ty} [{'+'.join(tags)}]")


# ---- capped launches -------------------------------------------------------------------------------------------------
CAPS = (128, 160, 100)      # the model's two shares and one that is no multiple of the tile columns


@pytest.mark.parametrize("ty", [1, 2])
@pytest.mark.parametrize("form", ["qkv", "fc1", "fc2", "proj", "gather256"])
def test_capped_launches(lib, ty, form):
    """max_wg: row blocks launched one after the other on the 256-row tiles (SAM qkv with its row map, fc1), the
    tile-walking kernel on 128 x 160 (fc2, proj with its A-row gather); gather256: the A-row gather and the aliased
    residual on 256^2 tiles, whose row blocks offset a_row_map and resid by hand.  Float64 on the uncapped run, then every
    capped run bit for bit against it."""
    M, N, K, tag = {"qkv": (4096, 3840, 1280, "256x256"), "fc1": (4096, 5120, 1280, "256x320"),
                    "fc2": (4096, 1280, 5120, "128x160s3"), "proj": (4096, 1280, 1280, "128x160s3"),
                    "gather256": (4096, 3840, 1280, "256x256")}[form]
    Msrc = 4900 if form in ("proj", "gather256") else M
    A, W, bias, resid, *_ = cu(*R.gemm_operands(Msrc, N, K, N + K))
    resid = resid[:, :M].contiguous()
    g = torch.Generator().manual_seed(N)
    rows_out, row_map, amap, kw = M, None, None, dict(bias=bias)
    if form == "qkv":        # tokens scattered into the window layout (4900 rows, the pad rows dropped by nobody here)
        rows_out = 4900
        row_map = torch.randperm(rows_out, generator=g)[:M].to(torch.int32).cuda()
        row_map[::11] = -1
        kw.update(row_map=row_map, C0=torch.full((1, rows_out, N), SENT, device="cuda"), c_f32=False)
    elif form == "fc1":
        kw.update(act=R.ACT_GELU, c_f32=False)
    else:
        kw.update(resid=resid)
        if form in ("proj", "gather256"):
            amap = torch.randperm(Msrc, generator=g)[:M].to(torch.int32).cuda()
            kw.update(a_row_map=amap)
    c_f32 = 0 if form in ("qkv", "fc1") else 1
    Ad, Wd = lay(A[0], K, adt(ty)), lay(W[0], K + 64, R.wdtype(ty))

    def run(cap):
        # fc2 / proj accumulate into the residual stream (resid == C)
        Cd = resid[0].clone() if c_f32 else torch.full((rows_out, N), SENT, dtype=adt(ty), device="cuda")
        tags, _ = gemm_ex(lib, ty, A=Ad, W=Wd, bias=bias[0], C=Cd, resid=Cd if c_f32 else None, row_map=row_map,
                          a_row_map=amap, M=M, N=N, K=K, lda=K, ldw=K + 64, ldc=N, ldr=N, c_f32=c_f32,
                          act=kw.get("act", 0), max_wg=cap)
        assert any(t.startswith(_PRE[ty]) and tag in t for t in tags), (tag, tags)
        return Cd
    base = run(0)
    ref, bound = R.gemm_form(ty, A, W, **kw)["C"]
    losses = ["drop_k"] + (["block_shift"] if tag.startswith("256") else [])
    muts = {k: R.gemm_form(ty, A, W, loss=k, block_rows=2048, **kw)["C"][0][0] for k in losses}
    R.check_bound(base, ref[0], bound[0], muts, f"capped {form} t={ty} uncapped")
    for cap in CAPS:
        assert torch.equal(run(cap), base), f"{form} t={ty}: max_wg = {cap} differs from the uncapped launch"


# ---- norm ------------------------------------------------------------------------------------------------------------
def norm_ex(lib, ty, **kw):
    from anyref_amd._lib import NormEx
    e = NormEx()
    for k, v in kw.items():
        setattr(e, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    call(lib, lib.anyref_op_norm_ex, ty, e)
    return e.fill_done


@pytest.mark.parametrize("ty", [1, 2, 3, 4])
@pytest.mark.parametrize("M,D,rms,act", [(4096, 1280, 0, 0), (333, 4096, 1, 0), (1000, 256, 0, R.ACT_GELU), (257, 1024, 0, 0),
                                         (77, 768, 0, 0), (50, 5120, 1, 0)])
def test_norm_typed_out_row_map_act(lib, ty, M, D, rms, act):
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * 3 + 1
    x[::5] *= 1e-3 / 3
    gain, bias = 1 + 0.2 * torch.randn(D, generator=g), torch.randn(D, generator=g)
    rows, ldy = M + 60, D + 64
    row_map = torch.randperm(rows, generator=g)[:M].to(torch.int32)
    row_map[::6] = -1
    x, gain, bias, row_map = cu(x, gain, bias, row_map)
    b = None if rms else bias
    yd = torch.full((rows, ldy), SENT, dtype=adt(ty), device="cuda")
    norm_ex(lib, ty, x=x, gain=gain, bias=b, y=yd, row_map=row_map, M=M, D=D, ldx=D, ldy=ldy, rms=rms, y_f32=0, act=act, eps=1e-6)
    kw = dict(rms=bool(rms), act=act, row_map=row_map, Y0=torch.full((rows, D), SENT, device="cuda"))
    ref, bound = R.norm_form(ty, x, gain, b, 1e-6, **kw)
    losses = ["row_map_ignored", "no_eps"] + (["act_dropped"] if act else [])
    muts = {n: R.norm_form(ty, x, gain, b, 1e-6, loss=n, **kw)[0] for n in losses}
    R.check_bound(yd[:, :D], ref, bound, muts, f"norm t={ty} {M}x{D} rms={rms} act={act}")
    assert (yd[:, D:] == SENT).all(), "y written past D"


@pytest.mark.parametrize("ty", [1, 2, 3, 4])
@pytest.mark.parametrize("D,fallback", [(1280, 0), (768, 0), (768, 1)])
def test_norm_fill_side_job(lib, ty, D, fallback):
    """the pad rows of a SAM window get the qkv bias from extra workgroups of norm1's launch (wide kernel, D >= 1024);
    a narrow norm leaves them alone (flag clear) and the model's fallback kernel writes them"""
    M, nfill, rows = 300, 41, 400
    g = torch.Generator().manual_seed(D)
    x = torch.randn(M, D, generator=g) * 3 + 1
    x[::5] *= 1e-3 / 3                                         # rows of magnitude ~ sqrt(eps): a norm without eps is far off there
    x, gain, bias = cu(x, 1 + 0.2 * torch.randn(D, generator=g), torch.randn(D, generator=g))
    fb = torch.randn(3 * D, generator=g).cuda()
    frows = torch.randperm(rows, generator=g)[:nfill].to(torch.int32).cuda()
    fdt = torch.float32 if ty in (3, 4) else adt(ty)           # (pairs mode: the attention that reads them takes f32)
    dst = torch.full((rows, 3 * D), SENT, dtype=fdt, device="cuda")
    yd = torch.full((M, D), SENT, dtype=adt(ty), device="cuda")
    done = norm_ex(lib, ty, x=x, gain=gain, bias=bias, y=yd, M=M, D=D, ldx=D, ldy=D, eps=1e-6, fill_dst=dst, fill_ld=3 * D,
                   fill_n=nfill, fill_N=3 * D, fill_rows=frows, fill_bias=fb, fill_fallback=fallback)
    assert done == (1 if D >= 1024 else 0)
    ref, bound = R.norm_form(ty, x, gain, bias, 1e-6)
    R.check_bound(yd, ref, bound, R.norm_form(ty, x, gain, bias, 1e-6, loss="no_eps")[0], f"norm beside fill t={ty} D={D}")
    dst0 = torch.full((rows, 3 * D), SENT, device="cuda")
    if not done and not fallback:
        assert (dst == SENT).all(), "fill rows written although the flag is clear"
        return
    gain3 = torch.cat([gain, gain, gain])
    ref, bound = R.fill_form(ty, dst0, frows, fb, 3 * D)
    muts = {n: R.fill_form(ty, dst0, frows, fb, 3 * D, gain=gain3, loss=n)[0] for n in ("gain_scaled", "rows_unmapped")}
    R.check_bound(dst, ref, bound, muts, f"fill rows t={ty} D={D} fallback={fallback}")


# ---- attention -------------------------------------------------------------------------------------------------------
def attn_ex(lib, ty, **kw):
    from anyref_amd._lib import AttnEx
    e = AttnEx()
    for k, v in kw.items():
        setattr(e, k, v if not isinstance(v, torch.Tensor) else v.data_ptr())
    return call(lib, lib.anyref_op_attention_ex, ty, e)


def _rel(qr, th, tw, size):
    """float64 decomposed rel-pos bias of the stored q, and sum |q| |R| of its dot products"""
    B, S, H, hd = qr.shape
    idx = (torch.arange(size)[:, None] - torch.arange(size)[None, :] + size - 1).cuda()
    rq = qr.double().permute(0, 2, 1, 3).reshape(B, H, size, size, hd)
    th, tw = th.double()[idx], tw.double()[idx]
    rel_h = torch.einsum("bnhwc,hkc->bnhwk", rq, th).reshape(B, H, S, size)
    rel_w = torch.einsum("bnhwc,wkc->bnhwk", rq, tw).reshape(B, H, S, size)
    rabs = [torch.einsum("bnhwc,hkc->bnhwk", rq.abs(), th.abs()).reshape(B, H, S, size),
            torch.einsum("bnhwc,wkc->bnhwk", rq.abs(), tw.abs()).reshape(B, H, S, size)]
    return rel_h, rel_w, rabs


_ATAG = {1: "attn_bf16_hd", 2: "attn_f16_hd", 3: "attn_sp16_hd"}


@pytest.mark.parametrize("ty", [1, 2, 3])
@pytest.mark.parametrize("form,B,H", [("window", 25, 16), ("global", 1, 16)])
def test_attention_fused_qkv_strides(lib, ty, form, B, H):
    """the SAM encoder's layout: q, k, v are column blocks of one [rows, 3 D] buffer (row stride 3 D), o rows at stride D;
    the 14 x 14 window with the rel-pos tables, the 64 x 64 global form with the P buffer; max_wg set and unset"""
    size, hd = (14, 80) if form == "window" else (64, 80)
    S, D = size * size, H * hd
    g = torch.Generator().manual_seed(S + H)
    qkv = torch.randn(B, S, 3 * D, generator=g).cuda().to(adt(ty))
    q, k, v = (qkv[..., i * D:(i + 1) * D].float().reshape(B, S, H, hd) for i in range(3))
    th, tw = (R.rnd(torch.randn(2 * size - 1, hd, generator=g) * 0.3, ty).cuda() for _ in range(2))
    rel_h, rel_w, rabs = _rel(q, th, tw, size)
    scale = hd ** -0.5
    kw = dict(q=qkv, k=C.c_void_p(qkv.data_ptr() + D * qkv.element_size()), v=C.c_void_p(qkv.data_ptr() + 2 * D * qkv.element_size()),
              q_bs=S * 3 * D, k_bs=S * 3 * D, v_bs=S * 3 * D, q_rs=3 * D, k_rs=3 * D, v_rs=3 * D, q_hs=hd, k_hs=hd, v_hs=hd,
              o_bs=S * D, o_rs=D, o_hs=hd, B=B, H=H, Sq=S, Sk=S, hd=hd, scale=scale, kh=size, kw=size)
    if form == "window":
        ld = 128
        tab = torch.zeros(2, 2 * size, ld, device="cuda")
        tab[0, : 2 * size - 1, :hd], tab[1, : 2 * size - 1, :hd] = th, tw
        tab = tab.to(adt(ty))
        kw.update(rel_tab_h=tab[0], rel_tab_w=tab[1], rel_tab_ld=ld)
        tile = 48
    else:
        npad = 2 * size
        p = torch.zeros(H, B * S, 2 * npad, device="cuda")
        qh = q.permute(2, 0, 1, 3).reshape(H, B * S, hd)
        p[:, :, : 2 * size - 1] = qh @ th.t()
        p[:, :, npad: npad + 2 * size - 1] = qh @ tw.t()
        kw.update(rel_p=p, rel_ld=2 * npad, rel_hs=B * S * 2 * npad)
        tile = 64
    outs = []
    for cap in (0, 128):
        o = torch.full((B, S, D), SENT, dtype=adt(ty), device="cuda")
        tags = attn_ex(lib, ty, o=o, max_wg=cap, **kw)
        # the form that ran: resident keys with the tables (16-bit windows), two query blocks per wave (16-bit global)
        want = "" if ty == 3 else "_res" if form == "window" else "_g2w"
        assert len(tags) == 1 and tags[0].startswith(_ATAG[ty] + "80") and want in tags[0], (want, tags)
        outs.append(o)
    assert torch.equal(outs[0], outs[1]), "max_wg changes the result"
    akw = dict(rel_h=rel_h, rel_w=rel_w, kw=size, rel_abs=rabs, rel_pairs=(ty == 3 and form == "window"), tile=tile)
    ref, bound = R.attention_form(ty, q, k, v, scale, **akw)
    muts = {n: R.attention_form(ty, q, k, v, scale, loss=n, k_wrong=q, **akw)[0] for n in ("drop_tile", "k_wrong")}
    R.check_bound(outs[0].reshape(B, S, H, hd), ref, bound, muts, f"attention fused qkv {form} t={ty} [{'+'.join(tags)}]")


@pytest.mark.parametrize("ty", [1, 2, 3])
def test_attention_prefill_from_cache_ragged(lib, ty):
    """prefill: keys and values read from the cache (batch stride maxS H hd != Sk H hd), causal, ragged q_len / kv_len over
    B = 4, two sequences with a cached prefix (q_pos0 > 0, so kv_len != q_len); rows >= q_len keep their sentinel exactly"""
    B, H, hd, S, maxS = 4, 8, 128, 320, 640
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, S, H, hd, generator=g).cuda().to(adt(ty))
    kc, vc = (torch.randn(B, maxS, H, hd, generator=g).cuda().to(adt(ty)) for _ in range(2))
    lens = torch.tensor([320, 257, 100, 1], dtype=torch.int32).cuda()
    p0 = torch.tensor([0, 30, 100, 0], dtype=torch.int32).cuda()
    kvl = lens + p0
    scale = hd ** -0.5
    outs = []
    for cap in (0, 128):
        o = torch.full((B, S, H, hd), SENT, dtype=adt(ty), device="cuda")
        tags = attn_ex(lib, ty, q=q, k=kc, v=vc, o=o, q_len=lens, kv_len=kvl, q_pos0=p0, q_bs=S * H * hd, q_rs=H * hd, q_hs=hd,
                       k_bs=maxS * H * hd, k_rs=H * hd, k_hs=hd, v_bs=maxS * H * hd, v_rs=H * hd, v_hs=hd, o_bs=S * H * hd,
                       o_rs=H * hd, o_hs=hd, B=B, H=H, Sq=S, Sk=S, hd=hd, scale=scale, causal=1, max_wg=cap)
        assert len(tags) == 1 and tags[0].startswith(_ATAG[ty] + "128"), tags
        outs.append(o)
    assert torch.equal(outs[0], outs[1]), "max_wg changes the result"
    kw = dict(causal=True, kv_len=kvl.cpu(), q_len=lens.cpu(), q_pos0=p0.cpu(), O0=torch.full((B, S, H, hd), SENT, device="cuda"))
    qf, kf, vf = q.float(), kc[:, :S].float(), vc[:, :S].float()
    ref, bound = R.attention_form(ty, qf, kf, vf, scale, **kw)
    muts = {n: R.attention_form(ty, qf, kf, vf, scale, loss=n, **kw)[0] for n in ("drop_tile", "q_len_ignored", "q_pos0_ignored")}
    R.check_bound(outs[0], ref, bound, muts, f"attention prefill from cache t={ty} [{'+'.join(tags)}]")
