"""The LoRA merge rule of adapter hot-swap (`anyref_adapter_apply`, csrc/lora.hip `lora_merge_rows_kernel`) in torch: what a
handle that reserved its LoRA targets stores after an adapter is applied.  It is stated the way `quant.py` states the fp8 and
int4 formats: the tests hold the device bits against these functions.

For a target with base `w` [N, K] (handed to `anyref_set_weight` in dtype `d_in`), `A` [r, K], `B` [N, r] (taken as f32; 16-bit
adapter tensors widen exactly) and `scaling = lora_alpha / r`:

    acc = 0 (f64);  for j = 0 .. r-1, in this order:  acc = acc + f64(B[n, j]) * f64(A[j, k])
    m   = f32(acc * f64(scaling) + f64(w[n, k]))      one f64 multiply, one f64 add, one round-to-nearest-even to f32
    m   = f32(d_in(m))                                the dtype the base was handed over in (merge_lora's `.to(w.dtype)`)
    stored = what finalize makes of an f32 tensor holding m   (RNE to the mode's weight type, or the fp8-row / int4-group quantiser)

Why f64: the product of two f32 values is exact in f64, so a fused multiply-add and a multiply followed by an add give the
same bits, and the explicit loop below reproduces the device bit for bit on any host.  The order of an f32 chain cannot be
restated in torch, and a host `b @ a` has no defined order.  `r = 0` (or a target an adapter does not name) gives the base
exactly as finalize converted it.

The rule is not bit-identical to `checkpoint.merge_lora` (which rounds `(b @ a) * scaling` to f32 first and sums in the BLAS
order): they differ in about 2e-4 of fp16 elements by one fp16 step.  `merge_lora` is unchanged.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Tuple

import torch

# projection name -> bit of `anyref_adapter_reserve`'s mask (include/anyref_hip.h ANYREF_LORA_*)
TARGET_BITS = {"q_proj": 1, "k_proj": 2, "v_proj": 4, "o_proj": 8, "gate_proj": 16, "up_proj": 32, "down_proj": 64}
MAX_RANK = 64


def parse_targets(adapters) -> int:
    """The `adapters=` argument of the model -> reservation mask: None -> 0 (no reservation), "qv" -> q_proj | v_proj (the
    reference's target_modules, train.py:371-374), or an iterable of projection names."""
    if adapters is None:
        return 0
    if isinstance(adapters, str):
        if adapters != "qv":
            raise ValueError(f'adapters={adapters!r}: pass None, "qv" or an iterable of projection names {sorted(TARGET_BITS)}')
        return TARGET_BITS["q_proj"] | TARGET_BITS["v_proj"]
    mask = 0
    for name in adapters:
        if name not in TARGET_BITS:
            raise ValueError(f"adapters: unknown projection {name!r} (one of {sorted(TARGET_BITS)})")
        mask |= TARGET_BITS[name]
    if not mask:
        raise ValueError("adapters: an empty list reserves nothing (pass None for a handle without adapters)")
    return mask


def target_bit(weight_name: str) -> int:
    """`model.layers.3.self_attn.q_proj.weight` -> its reservation bit (0: not a LLaMA linear)"""
    parts = weight_name.split(".")
    if len(parts) == 6 and parts[0] == "model" and parts[1] == "layers" and parts[5] == "weight":
        return TARGET_BITS.get(parts[4], 0)
    return 0


def merge_rule(w: torch.Tensor, a: Optional[torch.Tensor], b: Optional[torch.Tensor], scaling: float,
               fan_in_fan_out: bool = False) -> torch.Tensor:
    """-> the f32 tensor m [N, K] of the rule (after the `d_in` rounding; `d_in` = w.dtype).  a [r, K], b [N, r]; with
    `fan_in_fan_out` the adapter holds the transposed pair (a [r, N], b [K, r]) and delta = (b @ a).T, as in merge_lora."""
    d_in = w.dtype
    w = w.detach().cpu()
    if a is None or b is None or a.shape[0] == 0:
        return w.to(torch.float32)
    a, b = a.detach().cpu().to(torch.float32), b.detach().cpu().to(torch.float32)
    if fan_in_fan_out:                         # delta[n, k] = sum_j b[k, j] a[j, n] = sum_j a.T[n, j] b.T[j, k]
        a, b = b.t().contiguous(), a.t().contiguous()
    r = a.shape[0]
    if b.shape != (w.shape[0], r) or a.shape != (r, w.shape[1]):
        raise ValueError(f"LoRA pair shapes {tuple(b.shape)} x {tuple(a.shape)} do not match the base {tuple(w.shape)}")
    a64, b64 = a.to(torch.float64), b.to(torch.float64)
    acc = torch.zeros(w.shape, dtype=torch.float64)
    for j in range(r):
        acc = acc + b64[:, j:j + 1] * a64[j:j + 1, :]        # exact product, one f64 add
    m = (acc * torch.tensor(float(scaling), dtype=torch.float32).to(torch.float64) + w.to(torch.float64)).to(torch.float32)
    return m.to(d_in).to(torch.float32)


def device_pair(a: torch.Tensor, b: torch.Tensor, fan_in_fan_out: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The (A [r, K], B [N, r]) f32 pair `anyref_adapter_apply` is handed for an adapter's tensors."""
    a, b = a.detach().to(torch.float32), b.detach().to(torch.float32)
    if fan_in_fan_out:
        a, b = b.t(), a.t()
    return a.contiguous(), b.contiguous()


def merged_state_dict(sd: Dict[str, torch.Tensor], pairs: Dict[str, Tuple[torch.Tensor, torch.Tensor]],
                      saved: Dict[str, torch.Tensor], scaling: float, fan_in_fan_out: bool = False,
                      only: Optional[Iterable[str]] = None) -> Dict[str, torch.Tensor]:
    """The state dict a fresh handle must be built from to hold what `set_adapter` leaves on a reserved one: every LoRA
    target by the rule (kept in the base's dtype, which holds m exactly), `modules_to_save` tensors replaced.  `pairs` maps
    module names (`model.layers.0.self_attn.q_proj`) to (A, B)."""
    out = dict(sd)
    for mod, (a, b) in pairs.items():
        name = mod + ".weight"
        if only is not None and name not in only:
            continue
        w = sd[name]
        out[name] = merge_rule(w, a, b, scaling, fan_in_fan_out).to(w.dtype).to(w.device)
    for k, v in saved.items():
        out[k] = v
    return out
