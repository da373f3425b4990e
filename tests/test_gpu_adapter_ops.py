"""`lora_merge_rows_kernel` (csrc/lora.hip; entry `anyref_op_lora_merge`) against the torch statement of the merge rule
(anyref_amd/lora.py), bit for bit: every storage type, the destination layouts the handle uses (padded rows, the gate / up row
interleave), a base handed over in fp16, the register and the LDS form, and the two counters.  The quantised modes' path (f32
rows of the rule, then the quantiser finalize runs) is held against `quant.py` on the rule's f32."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anyref_amd import _lib  # noqa: E402
from anyref_amd.lora import merge_rule  # noqa: E402
from anyref_amd.quant import pack_groups_int4, quantize_groups_int4, quantize_rows_fp8  # noqa: E402

pytestmark = pytest.mark.gpu
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
TORCH_T = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
POISON = {0: 1234.5, 1: 1234.0, 2: 1234.0}      # exact in every type


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def inputs(N, K, r, d_in, seed):
    """base (exactly representable in d_in), A, B with the distribution of the issue's host measurement"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.02).to(TORCH_T[d_in])
    A = torch.randn(r, K, generator=g) * 0.05
    B = torch.randn(N, r, generator=g) * 0.05
    return w, A, B


def run_merge(lib, t, w, A, B, scaling, d_in, ld=None, row_stride=1, counts=False):
    """-> (dst rows [N * row_stride, ld] of type t as the device left them, counts [2] or None)"""
    N, K = w.shape
    ld = ld or K
    dst = torch.full((N * row_stride, ld), POISON[t], dtype=TORCH_T[t], device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda") if counts else None
    keep = [w.float().cuda().contiguous(), A.cuda().contiguous(), B.cuda().contiguous()]
    rc = lib.anyref_op_lora_merge(t, None, P(keep[0]), d_in, N, K, P(keep[1]), P(keep[2]), A.shape[0], scaling, P(dst), ld,
                                  row_stride, P(cnt) if counts else None)
    assert rc == 0, lib.anyref_op_last_error()
    torch.cuda.synchronize()
    return dst.cpu(), (cnt.cpu() if counts else None)


@pytest.mark.parametrize("t", [0, 1, 2])
@pytest.mark.parametrize("N,K,r,d_in,ld_extra,row_stride,scaling", [
    (40, 72, 1, 0, 64, 1, 2.0),             # padded rows: the pad is poisoned and must stay
    (256, 256, 4, 0, 0, 2, 16.0 / 13.0),    # gate / up interleave: the other rows poisoned and unchanged; inexact scaling
    (130, 688, 13, 2, 0, 1, 16.0 / 13.0),   # base handed over in fp16; odd rank, rows that are no multiple of the block's
    (64, 4096, 64, 0, 0, 1, 0.25),          # the LDS form at the full 7B row length
    (33, 20, 3, 1, 4, 1, 4.0),              # K % 8 != 0: the element-wise form; base handed over in bf16
])
def test_merge_bit_exact(t, N, K, r, d_in, ld_extra, row_stride, scaling):
    lib = _lib.load()
    w, A, B = inputs(N, K, r, d_in, seed=N * K + r)
    m = merge_rule(w, A, B, scaling)                       # f32 of the rule, after the d_in rounding
    want = m.to(TORCH_T[t])
    got, cnt = run_merge(lib, t, w, A, B, scaling, d_in, ld=K + ld_extra, row_stride=row_stride, counts=True)
    rows = got[::row_stride]
    assert torch.equal(bits(rows[:, :K]), bits(want))
    poison = torch.tensor(POISON[t], dtype=TORCH_T[t])
    assert (rows[:, K:] == poison).all(), "pad columns were written"
    if row_stride == 2:
        assert (got[1::2] == poison).all(), "the interleaved rows of the other tensor were written"
    if t != 0:                                             # elements whose stored value is not exactly m
        assert int(cnt[0]) == int((want.float() != m).sum()) and int(cnt[1]) == 0
    assert not torch.equal(m, w.float())                   # the adapter did change the tensor


@pytest.mark.parametrize("t", [0, 1, 2])
@pytest.mark.parametrize("r", [2, 24])                     # register form, LDS form
def test_zero_adapter_reproduces_the_converted_base(t, r):
    lib = _lib.load()
    w, A, B = inputs(96, 264, r, 0, seed=7 + r)
    w[0, 0] = 0.0
    got, _ = run_merge(lib, t, w, torch.zeros_like(A), B, 2.0, 0)
    assert torch.equal(bits(got), bits(w.to(TORCH_T[t])))


def test_f16_overflow_is_counted():
    lib = _lib.load()
    w, A, B = inputs(48, 64, 2, 0, seed=3)
    B[5, :] = torch.tensor([300.0, 0.0])
    A[0, 9] = 300.0                                        # 2 * 300 * 300 = 180000 > 65504; the rest of row 5 / column 9 stays small
    m = merge_rule(w, A, B, 2.0)
    over = m.abs() > 65504
    assert int(over.sum()) == 1 and bool(over[5, 9])
    got, cnt = run_merge(lib, 2, w, A, B, 2.0, 0, counts=True)
    assert int(cnt[1]) == 1
    assert torch.isinf(got[5, 9]) and int(torch.isinf(got).sum()) == 1
    _, cnt_bf = run_merge(lib, 1, w, A, B, 2.0, 0, counts=True)
    assert int(cnt_bf[1]) == 0                             # in range for bf16


def test_rank_outside_1_to_64_is_refused():
    lib = _lib.load()
    w, A, B = inputs(8, 16, 1, 0, seed=1)
    dst = torch.zeros(8, 16, device="cuda")
    keep = [w.cuda(), torch.zeros(65, 16).cuda(), torch.zeros(8, 65).cuda()]
    for r in (0, 65):
        rc = lib.anyref_op_lora_merge(0, None, P(keep[0]), 0, 8, 16, P(keep[1]), P(keep[2]), r, 1.0, P(dst), 16, 1, None)
        assert rc != 0 and b"outside 1 .. 64" in lib.anyref_op_last_error()
    assert lib.anyref_op_lora_merge(0, None, P(keep[0]), 0, 8, 16, P(keep[1]), P(keep[2]), 1, 1.0, P(dst), 8, 1, None) != 0  # ld < K
    assert lib.anyref_op_lora_merge(0, None, P(keep[0]), 0, 8, 16, P(keep[1]), P(keep[2]), 1, 1.0, P(dst), 16, 3, None) != 0  # stride


@pytest.mark.parametrize("d_in", [0, 2])
def test_quantised_path_equals_quantiser_of_the_rule(d_in):
    """perf_int4w / perf_fp8w: the kernel writes the rule's f32 rows into a scratch tensor and the quantiser finalize runs packs
    them (model.hip lora_write).  (128, 688): the last int4 group of a row is short."""
    lib = _lib.load()
    N, K, r, scaling = 128, 688, 8, 2.0
    w, A, B = inputs(N, K, r, d_in, seed=11)
    m = merge_rule(w, A, B, scaling)
    got, _ = run_merge(lib, 0, w, A, B, scaling, d_in)
    assert torch.equal(bits(got), bits(m))
    md = got.cuda()
    G = (K + 127) // 128
    nib = torch.empty(N, G * 64, dtype=torch.uint8, device="cuda")
    sc = torch.empty(N, G, dtype=torch.bfloat16, device="cuda")
    assert lib.anyref_op_quant_int4(None, P(md), N, K, P(nib), P(sc)) == 0, lib.anyref_op_last_error()
    q8 = torch.empty(N, K, dtype=torch.uint8, device="cuda")
    s8 = torch.empty(N, device="cuda")
    assert lib.anyref_op_quant_fp8(None, P(md), N, K, P(q8), P(s8)) == 0, lib.anyref_op_last_error()
    torch.cuda.synchronize()
    q_ref, s_ref = quantize_groups_int4(m)
    assert torch.equal(sc.cpu().float(), s_ref) and torch.equal(nib.cpu(), pack_groups_int4(q_ref))
    q8_ref, s8_ref = quantize_rows_fp8(m)
    assert torch.equal(s8.cpu(), s8_ref)
    # e4m3 has a -0: compare the bytes where the value is non-zero, the values everywhere
    a, b = q8.cpu(), q8_ref
    assert torch.equal(a.view(torch.float8_e4m3fn).float(), b.view(torch.float8_e4m3fn).float())
    nz = b.view(torch.float8_e4m3fn).float() != 0
    assert torch.equal(a[nz], b[nz])
