"""fp8 (OCP e4m3fn) weight-only quantisation of the LLaMA linear layers: the torch statement of what
`ANYREF_MODE_PERF_FP8W` does at `finalize` (csrc/ops.hip `quant_fp8_rows_kernel`).

    scale[n] = max_k |W[n, k]| / 448        (1 for an all-zero row)
    q[n, k]  = round-to-nearest-even_e4m3fn(W[n, k] / scale[n])
    W'[n, k] = float(q[n, k]) * scale[n]    <- what the fp8 path multiplies by

`dequantized_state_dict` gives a checker (the oracle) the weights the device computes with.
"""
import re
from typing import Dict, Tuple

import torch

FP8_MAX = 448.0
_LLM_LINEAR = re.compile(r"^(model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight|lm_head\.weight)$")


def quantize_rows_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] float -> (q uint8 [N, K] (e4m3fn bit patterns), scale f32 [N])."""
    w = w.detach().to(torch.float32)
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (w / scale[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def dequantize_rows_fp8(q_u8: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return q_u8.view(torch.float8_e4m3fn).to(torch.float32) * scale[:, None]


def is_fp8_weight(name: str) -> bool:
    """The tensors ANYREF_MODE_PERF_FP8W holds in fp8: q/k/v/o, gate/up/down of every layer, lm_head."""
    return _LLM_LINEAR.match(name) is not None


def dequantized_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in sd.items():
        if is_fp8_weight(k):
            q, s = quantize_rows_fp8(v.cpu())
            out[k] = dequantize_rows_fp8(q, s).to(v.dtype)
        else:
            out[k] = v
    return out


# ---- int4 group quantisation (ANYREF_MODE_PERF_INT4W; csrc/gemv_int4.hip `quant_int4_rows_kernel`) --------------------
#
#     groups of 128 consecutive k per output row (the last may be short; storage pads it with zeros)
#     amax = max |W[n, g]|;  amax < 2^-100: zero group, s = 1, q = 0
#     s    = amax / 7 (f32) rounded UP to 5 significant bits: a bf16 whose low 3 mantissa bits are zero
#     q    = clamp(rne(W / s), -7, 7)
#     W'   = q * s          <- |q| <= 7 has 3 significant bits, so W' is exactly a bf16
#
# lm_head stays bf16 (as AWQ / GPTQ checkpoints keep it).
INT4_GROUP = 128
INT4_QMAX = 7
_INT4_ZERO = 2.0 ** -100
_LLM_LINEAR_INT4 = re.compile(r"^model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight$")


def _scale_up_5bit(a: torch.Tensor) -> torch.Tensor:
    """positive f32 -> the smallest value >= a with 5 significant bits (sign, exponent, top 4 mantissa bits)"""
    u = a.contiguous().view(torch.int32)
    low = u & 0x7FFFF
    u = (u - low) + torch.where(low != 0, torch.full_like(u, 1 << 19), torch.zeros_like(u))
    return u.view(torch.float32)


def quantize_groups_int4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] float -> (q int8 [N, K] in -7 .. 7, s f32 [N, ceil(K / 128)], every s exactly a bf16)."""
    w = w.detach().to(torch.float32)
    N, K = w.shape
    G = (K + INT4_GROUP - 1) // INT4_GROUP
    wp = torch.zeros(N, G * INT4_GROUP, dtype=torch.float32)
    wp[:, :K] = w
    wg = wp.view(N, G, INT4_GROUP)
    amax = wg.abs().amax(dim=2)
    zero = amax < _INT4_ZERO
    s = _scale_up_5bit(torch.where(zero, torch.ones_like(amax), amax) / float(INT4_QMAX))
    s = torch.where(zero, torch.ones_like(s), s)
    q = torch.round(wg / s[:, :, None]).clamp_(-INT4_QMAX, INT4_QMAX)
    q = torch.where(zero[:, :, None], torch.zeros_like(q), q)
    return q.view(N, G * INT4_GROUP)[:, :K].to(torch.int8).contiguous(), s


def dequantize_groups_int4(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    K = q.shape[1]
    return q.to(torch.float32) * s.to(torch.float32).repeat_interleave(INT4_GROUP, dim=1)[:, :K]


def pack_groups_int4(q: torch.Tensor) -> torch.Tensor:
    """The reference statement of the device's nibble layout (what `quant_int4_rows_kernel` stores; the tests hold the device
    bytes against it): q int8 [N, K] in -7 .. 7 -> nibble rows uint8 [N, ceil(K / 128) * 64] (positions past K: q = 0).

    A nibble holds q + 8.  A dword is 8 consecutive weights: weight e sits at bit 4 * ((e >> 1) + 4 * (e & 1)), so that
    ((dword >> 4 j) & 0x000F000F) | 0x43004300 is the packed bf16 pair (136 + q[2 j], 136 + q[2 j + 1]); dwords are
    little-endian and in k order (a 16-byte block is 32 weights of one group)."""
    N, K = q.shape
    G = (K + INT4_GROUP - 1) // INT4_GROUP
    qp = torch.zeros(N, G * INT4_GROUP, dtype=torch.int64)
    qp[:, :K] = q
    shift = torch.tensor([4 * ((e >> 1) + 4 * (e & 1)) for e in range(8)], dtype=torch.int64)
    word = ((qp + 8).view(N, G * 16, 8) << shift).sum(-1)
    return torch.stack([(word >> (8 * b)) & 255 for b in range(4)], -1).to(torch.uint8).view(N, G * 64)


def is_int4_weight(name: str) -> bool:
    """The tensors ANYREF_MODE_PERF_INT4W holds in int4: q/k/v/o and gate/up/down of every layer (not lm_head)."""
    return _LLM_LINEAR_INT4.match(name) is not None


def dequantized_state_dict_int4(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in sd.items():
        if is_int4_weight(k):
            q, s = quantize_groups_int4(v.cpu())
            out[k] = dequantize_groups_int4(q, s).to(v.dtype)
        else:
            out[k] = v
    return out
