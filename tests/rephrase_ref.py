"""Float64 restatement of the fused rephrase launch pair (include/anyref_hip_ops.h `anyref_op_seg_rephrase`) and
the derived per-element bound tests/test_gpu_rephrase_ops.py holds the kernels to.  Plain torch on whatever device the
operands are on; nothing here needs a GPU or the HIP library (tests/test_cpu_rephrase_paths.py checks it against the oracle's
`generate_tail` on the CPU).

Conventions (tests/gemm_forms_ref.py): the reference is float64 over the operands AS STORED, so a product of two 16-bit
values is exact and the legitimate differences are f32 summation order, expf and the f32 divisions.  The bound is a sum of such
terms, each written down where it is added; none is tuned to what a kernel returns.
"""
import torch

U32 = 2.0 ** -24                      # unit roundoff of f32


def pass_a(q, K, e0, scale):
    """per-head attention of query row e0 over keys [0, e0]: q [heads, hd] (row e0 of one image), K [rows, heads, hd] -> p
    float64 [heads, e0 + 1], and the scaled absolute score products sum_d |q_d k_jd| * scale [heads, e0 + 1] (for the bound)"""
    q, k = q.double(), K[: e0 + 1].double()
    s = torch.einsum("hd,jhd->hj", q, k) * scale
    mag = torch.einsum("hd,jhd->hj", q.abs(), k.abs()) * scale
    return torch.softmax(s, dim=-1), mag


def pass_b(p, hidden, s0, e0, weight):
    """p [heads, e0 + 1] -> w_j = mean_h p_h[j] over the span [s0, e0), tot = sum_j w_j, the term weight * sum_j hidden[j] *
    (w_j / tot) float64 [D]; also weight * sum_j |hidden[j] * w_j| / tot (for the bound)"""
    w = p[:, s0:e0].mean(0)
    tot = w.sum()
    h = hidden[s0:e0].double()
    term = weight * (h * (w / tot)[:, None]).sum(0)
    mag = weight * (h.abs() * (w / tot)[:, None]).sum(0)
    return term, mag


def seg_rephrase(q_keep, kc, hidden, item, scale, weight):
    """one item (b, e0, s0, out_row) over q_keep / kc [B, maxS, heads, hd] and hidden [B, maxS, D] as stored -> (term, bound),
    both float64 [D]: what the pair adds to y[out_row] and how far an f32 implementation may be from it"""
    b, e0, s0, _ = item
    heads, hd = q_keep.shape[2], q_keep.shape[3]
    p, mag = pass_a(q_keep[b, e0], kc[b], e0, scale)
    term, tmag = pass_b(p, hidden[b], s0, e0, weight)
    return term, tmag * rel_bound(hd, heads, e0 + 1, e0 - s0, mag.max().item())


def rel_bound(hd, heads, n, span, max_score_mag):
    """Relative error of one term hidden_jd * w_j / tot of the sum, in f32:
      ds   = (hd + 2) * 2^-24 * max_j scale * sum_d |q_d k_jd|: an f32 dot of hd products in any order (hd roundings), the
             multiply by scale and the subtraction of the maximum (2) -- the absolute error of a score, which the exponential
             turns into a relative error of exp(score - max);
      w_j / tot is a ratio of two sums of p_h[j] = e_j / sum_j e_j: numerator and denominator each carry 2 * ds (e_j and the
             softmax sum, which lies between its terms' errors) plus the roundings of expf (2), the n-term sum (n), the division
             (1), the heads-term sum and the multiply by 1 / heads (heads + 1) and, for tot, the span-term sum, folded with the
             final division into the last summand: 2 * (2 * ds + (n + heads + 6) * 2^-24);
      the weighted sum over the span: span fmas, the division w_j / tot, the multiply by the weight and the add into y:
             (2 * span + 2) * 2^-24."""
    ds = (hd + 2) * U32 * max_score_mag
    return 2 * (2 * ds + (n + heads + 6) * U32) + (2 * span + 2) * U32
