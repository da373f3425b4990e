"""The int4 group format of `perf_int4w` as `anyref_amd/quant.py` states it (CPU): the properties the kernels and the
oracle comparison rest on -- W' = q * s is exactly a bf16, so there is one set of weights and no second rounding."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anyref_amd.quant import (INT4_GROUP, dequantize_groups_int4, dequantized_state_dict_int4, is_fp8_weight,  # noqa: E402
                              is_int4_weight, quantize_groups_int4)


def weights(N, K, kind, seed=0):
    g = torch.Generator().manual_seed(seed + N * 131 + K)
    w = torch.randn(N, K, generator=g) * 0.02
    if kind == "zero_row":
        w[0] = 0
        w[1, : min(K, INT4_GROUP)] = 0                     # one zero group inside a live row
    elif kind == "outlier":
        w[1, 0] = 3.0
        w[2, K - 1] = -5.0
        w[3, :8] = torch.tensor([1e-9, -1e-9, 5e-5, -5e-5, 0.02, -0.02, 1e-3, 7e-4])[: min(8, K)]
    elif kind == "tiny":
        w = w * 2.0 ** -90                                 # around the zero-group threshold 2^-100
    return w


@pytest.mark.parametrize("kind", ["random", "zero_row", "outlier", "tiny"])
@pytest.mark.parametrize("N,K", [(16, 256), (9, 688), (5, 16), (4, 4096), (4, 11008)])
def test_format_properties(N, K, kind):
    w = weights(N, K, kind)
    q, s = quantize_groups_int4(w)
    G = (K + INT4_GROUP - 1) // INT4_GROUP
    assert q.shape == (N, K) and q.dtype == torch.int8 and s.shape == (N, G) and s.dtype == torch.float32
    wd = dequantize_groups_int4(q, s)
    assert torch.equal(wd.bfloat16().float(), wd), "W' is not bf16-exact"
    assert torch.equal(s.bfloat16().float(), s), "s is not bf16-exact"
    assert ((s.view(torch.int32) & 0x7FFFF) == 0).all(), "s has more than 5 significant bits"
    pad = torch.zeros(N, G * INT4_GROUP)
    pad[:, :K] = w
    amax = pad.view(N, G, INT4_GROUP).abs().amax(2)
    qp = torch.zeros(N, G * INT4_GROUP, dtype=torch.int8)
    qp[:, :K] = q
    qmax = qp.view(N, G, INT4_GROUP).abs().amax(2)
    zero = amax < 2.0 ** -100
    assert torch.equal(s[zero], torch.ones_like(s[zero])) and (qmax[zero] == 0).all()
    nz = ~zero
    lo = amax[nz] / 7.0
    assert (s[nz] >= lo).all() and (s[nz].double() <= 1.0625 * lo.double()).all()
    assert (qmax[nz] == 7).all(), "a nonzero group does not reach |q| = 7"
    se = s.repeat_interleave(INT4_GROUP, dim=1)[:, :K]
    live = (~zero).repeat_interleave(INT4_GROUP, dim=1)[:, :K]
    assert ((w - wd).abs()[live].double() <= se[live].double() / 2).all()
    q2, s2 = quantize_groups_int4(wd)
    assert torch.equal(q2, q) and torch.equal(s2, s), "quantising W' is not idempotent"


def test_hand_example():
    w = torch.zeros(1, 128)
    w[0, :3] = torch.tensor([0.07, -0.035, 0.0101])
    q, s = quantize_groups_int4(w)
    assert s.item() == 0.01025390625 == 0b10101 * 2.0 ** -11
    assert q[0, :3].tolist() == [7, -3, 1] and (q[0, 3:] == 0).all()


def test_names():
    assert is_int4_weight("model.layers.0.self_attn.q_proj.weight") and is_int4_weight("model.layers.31.mlp.down_proj.weight")
    assert not is_int4_weight("lm_head.weight") and is_fp8_weight("lm_head.weight")
    assert not is_int4_weight("model.embed_tokens.weight")
    sd = {"lm_head.weight": torch.randn(4, 128), "model.layers.0.mlp.up_proj.weight": torch.randn(4, 128).bfloat16()}
    dq = dequantized_state_dict_int4(sd)
    assert dq["lm_head.weight"] is sd["lm_head.weight"]
    assert dq["model.layers.0.mlp.up_proj.weight"].dtype == torch.bfloat16
    assert not torch.equal(dq["model.layers.0.mlp.up_proj.weight"], sd["model.layers.0.mlp.up_proj.weight"])


def test_mode_code_in_header_and_ctypes():
    from anyref_amd import _lib
    txt = open(os.path.join(ROOT, "include", "anyref_hip.h")).read()
    codes = {n: int(v) for n, v in re.findall(r"#define\s+ANYREF_MODE_(\w+)\s+\(?(\d+)\)?", txt)}
    assert codes["PERF_INT4W"] == 6 == _lib.MODE_PERF_INT4W
    assert sorted(codes.values()) == list(range(7)), codes          # seven modes, no code used twice
    v = re.search(r"#define\s+ANYREF_ABI_VERSION\s+(\d+)", txt)
    assert v and int(v.group(1)) == 2 == _lib.ABI_VERSION           # anyref_config is unchanged
