"""Golden vectors that pin the mask-report rule (`anyref_amd/maskreport.py`) to the reference's own
`calculate_stability_score`, `batched_mask_to_box` and `mask_to_rle_pytorch`
(`model/segment_anything/utils/amg.py`), imported by path and called at SAM's defaults (mask threshold 0, offset 1).

Run ONLY where the reference is at hand (it never travels):

    python tests/golden/make_golden_mask_report.py [/path/to/reference]

Writes `tests/golden/mask_report_amg.npz`, data only: per case the seeded f32 logits with the special values planted (exact
0.0, -0.0, +-offset, NaN, +-inf, an all-negative mask, a mask wholly below -offset), and what the three reference functions
returned for them -- stability f32 (NaN included), boxes, and the RLE counts flattened with their lengths.  No reference source
is stored.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OFFSET = 1.0
SHAPES = [(1, 1, 1), (1, 3, 31), (1, 5, 33), (2, 7, 63), (1, 9, 65), (1, 2, 129), (3, 37, 101)]
SPECIALS = [0.0, -0.0, OFFSET, -OFFSET, float("nan"), float("inf"), float("-inf")]


def planted_logits(n, H, W, seed):
    """normal x 2 with every special value planted in every mask that has room, at seeded places (the last column among them)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, H, W)) * 2).astype(np.float32)
    for m in range(n):
        flat = x[m].reshape(-1)
        k = min(len(SPECIALS) * 2, flat.size)
        where = rng.choice(flat.size, size=k, replace=False)
        for i, p in enumerate(where):
            flat[p] = SPECIALS[i % len(SPECIALS)]
        if H * W >= 4:
            x[m, H - 1, W - 1] = 0.5        # the last bit of the last word
            x[m, 0, W - 1] = 0.0
    if (n, H, W) == (1, 1, 1):
        x[0, 0, 0] = 0.0                    # exactly the threshold: an empty mask whose area_lo is 1
    if (n, H, W) == (2, 7, 63):
        x[1] = -3.0                         # wholly below -offset: area_lo = 0, stability NaN
        x[1, 3, 5] = float("nan")
    if (n, H, W) == (3, 37, 101):
        x[1] = -np.abs(x[1]) * np.float32(0.25)     # all-negative: empty, box 0 0 0 0 (NaN, -0.0 and -inf stay in it)
    return x


def main():
    spec = importlib.util.spec_from_file_location("ref_amg", os.path.join(REF, "model/segment_anything/utils/amg.py"))
    amg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(amg)
    out = {"offset": np.float32(OFFSET), "shapes": np.array(SHAPES, dtype=np.int64)}
    for i, (n, H, W) in enumerate(SHAPES):
        x = planted_logits(n, H, W, seed=100 + i)
        t = torch.from_numpy(x)
        stab = amg.calculate_stability_score(t, 0.0, OFFSET)
        boxes = amg.batched_mask_to_box(t > 0.0)
        rles = amg.mask_to_rle_pytorch(t > 0.0)
        assert all(r["size"] == [H, W] for r in rles)
        out[f"logits_{i}"] = x
        out[f"stability_{i}"] = stab.numpy().astype(np.float32)
        out[f"boxes_{i}"] = boxes.numpy().astype(np.int64)
        out[f"rle_counts_{i}"] = np.array([c for r in rles for c in r["counts"]], dtype=np.int64)
        out[f"rle_lens_{i}"] = np.array([len(r["counts"]) for r in rles], dtype=np.int64)
    path = os.path.join(HERE, "mask_report_amg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
