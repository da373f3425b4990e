"""The token-score rule (include/anyref_hip.h `anyref_set_token_scores`), stated once in plain numpy float64:
what `token_scores_kernel` (csrc/ops.hip) computes on the device from the f32 logits row that decided a generated token.
Nothing here touches the GPU; the CPU tests hold the rule to `torch.log_softmax` / `torch.topk`, the GPU tests hold the kernel
and the model's bookkeeping to the rule.

For a row x of N >= 2 f32 logits:
  id      = the first index of the maximum, NaN counting as the greatest value -- the order `argmax_kernel` documents, so id
            always equals the emitted token;
  logprob = x[id] - lse,  lse = m + log(sum_i exp(x_i - m)),  m = x[id]      (float64 here, f32 on the device);
  gap     = x[id] - second, the f32 subtraction, second = the greatest value among the indices other than id: the top-2
            logit gap, 0 on a tie.
A row holding a NaN gives logprob = gap = NaN.  -inf entries add 0 to the sum.  Whatever else IEEE arithmetic gives for the
formula stands: a row of -inf (m - m = NaN) gives NaN, and so does the logprob of a row holding +inf.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def _f32_row(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise TypeError(f"token_scores_rule takes an f32 logits row, got {x.dtype}")
    if x.ndim != 1 or x.shape[0] < 2:
        raise ValueError("token_scores_rule takes one row of N >= 2 logits")
    return x


def token_scores_rule(x_f32_row) -> Tuple[int, float, float]:
    """-> (id, logprob, gap) of one f32 logits row (a 1-D torch tensor or numpy array)."""
    x = _f32_row(x_f32_row)
    nan = np.isnan(x)
    i = int(np.argmax(nan)) if nan.any() else int(np.argmax(x))     # np.argmax: the first occurrence
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        m = x64[i]
        lse = m + np.log(np.sum(np.exp(x64 - m)))
        logprob = x64[i] - lse
        second = np.max(np.delete(x, i))
        gap = np.float32(x[i]) - np.float32(second)
    return i, float(logprob), float(gap)


def token_scores_rows(x_f32_rows):
    """the rule on every row of a [M, N] f32 matrix -> (ids i64 [M], logprob f64 [M], gap f32 [M]) numpy arrays"""
    if hasattr(x_f32_rows, "detach"):
        x_f32_rows = x_f32_rows.detach().cpu().numpy()
    rows = [token_scores_rule(r) for r in np.asarray(x_f32_rows)]
    return (np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.float64),
            np.array([r[2] for r in rows], dtype=np.float32))
