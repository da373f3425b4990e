"""The int4-operand GEMM's public surface and its fragment identity, without a GPU: the library exports
`anyref_op_gemm_int4` as `_lib` declares it, and a torch statement of what the kernel does with one LDS dword -- unpack the
eight nibbles as packed bf16 pairs (136 + q), widen to f32, fma with the group scale -- gives exactly the bf16 values
`q * s` of `dequantize_groups_int4`, in k order; so does the byte route (q + 8) the GEMM kernel takes to the same values."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anyref_amd import _lib  # noqa: E402
from anyref_amd.quant import dequantize_groups_int4, pack_groups_int4, quantize_groups_int4  # noqa: E402


def test_library_exports_gemm_int4_as_declared():
    """(stream, A, W4, scale_bf16, bias, C, resid, M, N, K, act, c_f32, swiglu) -> int"""
    res, args = _lib.SYMBOLS["anyref_op_gemm_int4"]
    assert res is C.c_int
    assert args == [C.c_void_p] * 7 + [C.c_int] * 6
    lib = C.CDLL(_lib.LIB_PATH)       # dlopen only: no device is touched
    assert hasattr(lib, "anyref_op_gemm_int4")
    header = open(os.path.join(ROOT, "include", "anyref_hip_ops.h")).read()
    assert "int anyref_op_gemm_int4(void* stream, const void* A, const uint8_t* W4, const void* scale_bf16," in header


def kernel_unpack(dwords):
    """int64 dwords [...] -> f32 [..., 8]: pair j is ((dw >> 4 j) & 0x000F000F) | 0x43004300, a packed bf16 pair whose low
    half is element 2 j and whose high half is element 2 j + 1; each half widened to f32 (16-bit shift)"""
    out = []
    for j in range(4):
        p = ((dwords >> (4 * j)) & 0x000F000F) | 0x43004300
        for half in (p & 0xFFFF, p >> 16):
            out.append((half << 16).to(torch.int32).view(torch.float32))
    return torch.stack(out, -1)


def gemm_unpack(dwords):
    """the GEMM's route to the same eight values: the even nibbles (dw & 0x0F0F0F0F) and the odd ones ((dw >> 4) & 0x0F0F0F0F)
    one per byte; byte b of the even set is weight {0, 4, 1, 5}[b], of the odd set {2, 6, 3, 7}[b]; int64 dwords -> q + 8"""
    ev, od = dwords & 0x0F0F0F0F, (dwords >> 4) & 0x0F0F0F0F
    by = lambda x, b: ((x >> (8 * b)) & 0xFF).float()  # noqa: E731
    pairs = [(ev, 0), (od, 0), (ev, 1), (od, 1)]       # output pair j = weights (2 j, 2 j + 1) = bytes (b, b + 2)
    return torch.stack([by(x, b + h) for x, b in pairs for h in (0, 2)], -1)


def test_dword_unpack_gives_the_quantised_values_in_k_order():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(9, 320, generator=g) * 0.05          # 2.5 groups: the last block row is padded with q = 0
    q, s = quantize_groups_int4(w)
    rows = pack_groups_int4(q)
    assert rows.shape == (9, 3 * 64) and rows.dtype == torch.uint8
    b = rows.to(torch.int64).view(9, -1, 4)
    dwords = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (b[..., 3] << 24)
    P = kernel_unpack(dwords).view(9, -1)                # 136 + q, k order
    assert torch.equal(P[:, :320], q.float() + 136)
    assert torch.equal(P[:, 320:], torch.full((9, 64), 136.0))
    assert torch.equal(gemm_unpack(dwords).view(9, -1), P - 128)     # the GEMM's byte route: q + 8, same order


def test_fragment_identity_all_nibbles_and_5bit_scales():
    """fma(136 + q, s, -136 s): the product has 8 x 5 significant bits (exact in f32), -136 s is exact (5 x 5 bits), the
    sum cancels to q * s exactly; its low 16 bits are zero, so truncating to the high half is the bf16 q * s"""
    nib = torch.arange(1, 16, dtype=torch.int64)         # the 15 nibbles the quantiser writes (q = -7 .. 7)
    q = (nib - 8).float()
    # every 5-significant-bit scale over a wide exponent range: sign 0, exponent e, top 4 mantissa bits m
    e = torch.arange(127 - 60, 127 + 20, dtype=torch.int64)
    m = torch.arange(16, dtype=torch.int64)
    s = ((e[:, None] << 23) | (m[None, :] << 19)).to(torch.int32).view(torch.float32).reshape(-1)
    assert torch.equal(s.bfloat16().float(), s)
    dw = nib | (nib << 16)                               # both halves of pair 0 hold the nibble
    P = kernel_unpack(dw)[:, 0]
    assert torch.equal(P, q + 136)
    Pd, sd = P.double()[:, None], s.double()[None, :]
    assert torch.equal((P[:, None] * s[None, :]).double(), Pd * sd), "136 + q times s is not exact in f32"
    neg = (-136.0 * s)
    assert torch.equal(neg.double(), -136.0 * s.double())
    v = (Pd * sd + neg.double()[None, :]).float()        # the fma: one rounding of the exact sum -- which is representable
    assert torch.equal(v.double(), Pd * sd + neg.double()[None, :])
    bits = v.view(torch.int32)
    assert (bits & 0xFFFF).eq(0).all()
    want = dequantize_groups_int4((nib - 8).to(torch.int8)[:, None], torch.ones(15, 1))  # q itself
    got_bf16 = (bits >> 16).to(torch.int16).view(torch.bfloat16)
    ref = (want * s[None, :]).bfloat16()
    assert torch.equal(ref.float(), want * s[None, :])
    nz = ref != 0
    assert torch.equal(got_bf16.view(torch.int16)[nz], ref.view(torch.int16)[nz])
    assert torch.equal(got_bf16.float(), ref.float())
    assert (bits[q == 0] == 0).all()                     # q = 0 widens to +0, as the image kernel writes it
    # the GEMM widens through fma(q + 8, s, -8 s) (4 x 5 bits, then the same exact cancellation): the same f32 bits
    B = gemm_unpack(dw)[:, 0]
    assert torch.equal(B, q + 8)
    v8 = (B.double()[:, None] * sd + (-8.0 * s).double()[None, :]).float()
    assert torch.equal(v8.double(), B.double()[:, None] * sd - 8.0 * sd)
    assert torch.equal(v8.view(torch.int32), bits)
