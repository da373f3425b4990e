"""SAM's spatial prompts, stated once on the CPU: the rule the HIP prompt kernels and the C entries are tested against.

Plain torch, float64 where it computes.  `encode` follows the reference's `PromptEncoder`
(`model/segment_anything/modeling/prompt_encoder.py:78-186`), `pick` its output selection
(`mask_decoder.py:106-112`, `convert_avs_masks.py:61-65`), `to_input_frame` the coordinate half of `ResizeLongestSide`
(`utils/transforms.py:36-66`).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

PE_PREFIX = "model.visual_model.prompt_encoder."

SPATIAL_NAMES = tuple(
    [f"point_embeddings.{i}.weight" for i in range(4)] + ["not_a_point_embed.weight"] +
    [f"mask_downscaling.{i}.{p}" for i in (0, 1, 3, 4, 6) for p in ("weight", "bias")])


def _pe(w, cfg, xy: torch.Tensor) -> torch.Tensor:
    """xy [..., 2] pixels of the SAM input frame, already shifted to the pixel centre -> [..., C]"""
    G = w[PE_PREFIX + "pe_layer.positional_encoding_gaussian_matrix"].double()
    c = xy.double() / cfg.sam.img_size
    v = 2 * math.pi * ((2 * c[..., 0:1] - 1) * G[0] + (2 * c[..., 1:2] - 1) * G[1])
    return torch.cat([torch.sin(v), torch.cos(v)], -1)


def _ln2d(x, weight, bias, eps=1e-6):
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return weight[None, :, None, None] * ((x - u) / torch.sqrt(s + eps)) + bias[None, :, None, None]


def mask_downscaling(w, mask_input: torch.Tensor) -> torch.Tensor:
    """mask_input [n, 4g, 4g] -> [n, C, g, g]: conv k2s2, LayerNorm2d eps 1e-6, exact-erf GELU, conv k2s2, LayerNorm2d, GELU,
    conv 1x1 (prompt_encoder.py:55-64)"""
    p = PE_PREFIX + "mask_downscaling."
    d = lambda k: w[p + k].double()
    x = mask_input.double()[:, None]
    x = F.gelu(_ln2d(F.conv2d(x, d("0.weight"), d("0.bias"), stride=2), d("1.weight"), d("1.bias")))
    x = F.gelu(_ln2d(F.conv2d(x, d("3.weight"), d("3.bias"), stride=2), d("4.weight"), d("4.bias")))
    return F.conv2d(x, d("6.weight").reshape(d("6.weight").shape[0], -1, 1, 1), d("6.bias"))


def encode(weights: Dict[str, torch.Tensor], cfg, points: Optional[torch.Tensor], labels: Optional[torch.Tensor],
           boxes: Optional[torch.Tensor], mask_input: Optional[torch.Tensor], text: Optional[torch.Tensor]
           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (sparse [n, Ns, C], dense [n, C, g, g]), float64.

    points [n, P, 2] (x, y) and boxes [n, 4] (x0 y0 x1 y1) in pixels of the SAM input frame, labels [n, P] (1 foreground,
    0 background, -1 not a point), mask_input [n, 4g, 4g], text [n, C] or [n, 1, C].  A coordinate p becomes
    c = (p + 0.5) / sam_img, v = 2 pi ((2 c_x - 1) G0 + (2 c_y - 1) G1), and the token is sin v | cos v.  Label 1 adds
    point_embeddings.1, label 0 point_embeddings.0, label -1 gives 0 + not_a_point_embed, any other label the PE alone (as
    the reference does).  One padding point (coordinate 0, label -1) is appended iff points are given and boxes are not.
    Box corners add point_embeddings.2 / .3.  Token order: points, pad, box corners, text."""
    C, g = cfg.sam.out_chans, cfg.sam.grid
    e = lambda k: weights[PE_PREFIX + k].double().reshape(-1)
    n = next((t.shape[0] for t in (points, boxes, mask_input, text) if t is not None), 1)
    parts = []
    if points is not None:
        assert labels is not None, "points without labels"
        pts, lab = points.double() + 0.5, labels.to(torch.int64)
        if boxes is None:
            pts = torch.cat([pts, torch.zeros(n, 1, 2, dtype=torch.float64)], 1)
            lab = torch.cat([lab, -torch.ones(n, 1, dtype=torch.int64)], 1)
        t = _pe(weights, cfg, pts)
        t = torch.where((lab == -1)[..., None], torch.zeros_like(t) + e("not_a_point_embed.weight"), t)
        t = t + (lab == 0)[..., None] * e("point_embeddings.0.weight") + (lab == 1)[..., None] * e("point_embeddings.1.weight")
        parts.append(t)
    if boxes is not None:
        t = _pe(weights, cfg, boxes.double().reshape(n, 2, 2) + 0.5).clone()
        t[:, 0] += e("point_embeddings.2.weight")
        t[:, 1] += e("point_embeddings.3.weight")
        parts.append(t)
    if text is not None:
        parts.append(text.double().reshape(n, 1, C))
    sparse = torch.cat(parts, 1) if parts else torch.zeros(n, 0, C, dtype=torch.float64)
    if mask_input is not None:
        dense = mask_downscaling(weights, mask_input)
    else:
        dense = e("no_mask_embed.weight").reshape(1, C, 1, 1).expand(n, C, g, g)
    return sparse, dense


def to_input_frame(coords_xy, orig_hw: Sequence[int], resized_hw: Sequence[int]) -> torch.Tensor:
    """Original-image pixels -> pixels of the SAM input frame: x * (new_w / old_w), y * (new_h / old_h), computed in float64
    and then rounded to f32.  Boxes go through as their two corners (reshape to [..., 2] first).

    This restates `ResizeLongestSide.apply_coords` (`utils/transforms.py:36-66`).  That file imports torchvision, which the
    machine the fixtures were made on does not have, so this one step is NOT pinned by a golden vector: it is checked on
    hand-computed values only (tests/test_cpu_prompts.py)."""
    c = torch.as_tensor(coords_xy, dtype=torch.float64).clone()
    assert c.shape[-1] == 2, "coordinates are (x, y) pairs"
    old_h, old_w = int(orig_hw[0]), int(orig_hw[1])
    new_h, new_w = int(resized_hw[0]), int(resized_hw[1])
    c[..., 0] = c[..., 0] * (new_w / old_w)
    c[..., 1] = c[..., 1] * (new_h / old_h)
    return c.to(torch.float32)


def pick(iou: torch.Tensor, multimask: bool):
    """iou [..., 4] -> (tokens, best): `multimask_output=False` gives token 0; True gives tokens 1..3 and best = argmax of
    their predicted IoU, as an index into the three returned masks."""
    if not multimask:
        return slice(0, 1), torch.zeros(iou.shape[:-1], dtype=torch.int64)
    return slice(1, 4), torch.argmax(iou[..., 1:4], -1)
