"""The mask-report rule (include/anyref_hip.h `anyref_set_mask_reports`), stated once in plain numpy on the CPU:
what `mask_report_kernel` (csrc/mask_report.hip) computes on the device from the f32 mask logits a call wrote to `out_masks`.
Nothing here touches the GPU; the CPU tests hold the rule to the reference's `calculate_stability_score`,
`batched_mask_to_box` and `mask_to_rle_pytorch` through recorded fixtures, the GPU tests hold the kernel and the model's
bookkeeping to the rule.  The rule is exact: integer counts, no tolerance anywhere.

For one mask x, f32 logits [H, W], and an f32 offset d >= 0 (default 1.0; the mask threshold is 0 -- SAM's defaults):
  bit(y, x)  = x > 0                 the project's reading of sigmoid > 0.5 (iou_counts_kernel); NaN gives 0, -0.0 gives 0
  area       = #{x > 0}      area_hi = #{x > +d}      area_lo = #{x > -d}
  nonfinite  = #{x is NaN or +-inf}  the health flag of the f16 modes, whose saturation shows as NaN
  box        = x0, y0, x1, y1: inclusive XYXY of the set bits, 0, 0, 0, 0 for an empty mask
  stability  = float32(area_hi) / float32(area_lo), NaN when area_lo == 0   (derived on the host)
  packed     = uint32 [H, Wp], Wp = ceil(W / 32): bit k of word w of row y is bit(y, 32 w + k), LSB first; bits past W are 0
The record that leaves the device is int32[8] = {area, area_hi, area_lo, nonfinite, x0, y0, x1, y1}; torch carries the packed
words as int32 with the same bit pattern.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np


def _f32_masks(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise TypeError(f"mask_report_rule takes f32 logits, got {x.dtype}")
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("mask_report_rule takes logits [H, W] or [n, H, W] with H, W >= 1")
    return x


def packed_width(W: int) -> int:
    return (int(W) + 31) // 32


def pack_bits(bits) -> np.ndarray:
    """bool [n, H, W] -> uint32 [n, H, Wp], LSB first, bits past W zero"""
    bits = np.asarray(bits, dtype=bool)
    n, H, W = bits.shape
    Wp = packed_width(W)
    padded = np.zeros((n, H, Wp * 32), dtype=np.uint64)
    padded[:, :, :W] = bits
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (padded.reshape(n, H, Wp, 32) * weights).sum(-1).astype(np.uint32)


def mask_report_rule(logits_f32, offset: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """-> (records int32 [n, 8], packed uint32 [n, H, Wp]) of f32 logits [n, H, W] (or [H, W]: n = 1)."""
    x = _f32_masks(logits_f32)
    d = np.float32(offset)
    if not np.isfinite(d) or d < 0:
        raise ValueError("mask_report_rule: the offset must be finite and >= 0")
    n, H, W = x.shape
    rec = np.zeros((n, 8), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        bits = x > np.float32(0)
        rec[:, 0] = bits.sum((1, 2))
        rec[:, 1] = (x > d).sum((1, 2))
        rec[:, 2] = (x > -d).sum((1, 2))
    rec[:, 3] = (~np.isfinite(x)).sum((1, 2))
    for i in range(n):
        ys, xs = np.nonzero(bits[i])
        if ys.size:
            rec[i, 4:] = (xs.min(), ys.min(), xs.max(), ys.max())
    return rec, pack_bits(bits)


def stability(records) -> np.ndarray:
    """f32 [n]: float32(area_hi) / float32(area_lo), NaN where area_lo == 0 (calculate_stability_score's own answer there)"""
    rec = np.asarray(records).reshape(-1, 8)
    with np.errstate(invalid="ignore", divide="ignore"):
        return rec[:, 1].astype(np.float32) / rec[:, 2].astype(np.float32)


def _words(packed) -> np.ndarray:
    if hasattr(packed, "detach"):
        packed = packed.detach().cpu().numpy()
    p = np.asarray(packed)
    if p.dtype == np.int32:
        p = p.view(np.uint32)
    if p.dtype != np.uint32:
        raise TypeError(f"packed masks are uint32 (or int32 of the same bits), got {p.dtype}")
    if p.ndim == 2:
        p = p[None]
    if p.ndim != 3:
        raise ValueError("packed masks are [H, Wp] or [n, H, Wp]")
    return p


def unpack(packed, W: int) -> np.ndarray:
    """packed [n, H, Wp] (uint32, or torch / numpy int32 of the same bits) -> bool [n, H, W]"""
    p = _words(packed)
    n, H, Wp = p.shape
    if Wp != packed_width(W):
        raise ValueError(f"a mask {W} wide packs into {packed_width(W)} words per row, got {Wp}")
    bits = (p[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(n, H, Wp * 32)[:, :, :W].astype(bool)


def rle(packed, W: int) -> List[Dict[str, list]]:
    """One uncompressed COCO RLE per mask, {"size": [H, W], "counts": [...]}: column-major runs starting with the zero run, as
    `mask_to_rle_pytorch` gives them."""
    out = []
    for m in unpack(packed, W):
        H = m.shape[0]
        flat = m.T.reshape(-1)
        change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
        edges = np.concatenate([[0], change, [H * W]])
        counts = ([0] if flat[0] else []) + np.diff(edges).tolist()
        out.append({"size": [H, int(W)], "counts": counts})
    return out
