"""Adapter hot-swap without a GPU: the merge rule (anyref_amd/lora.py) against the host merge it stands beside, its identities,
the adapter parser split out of `merge_lora`, the declared / bound entries, and the Python state rules."""
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anyref_amd.config import config_tiny  # noqa: E402
from anyref_amd.synth import synth_state_dict  # noqa: E402
from test_cpu_checkpoint import _write_adapter  # noqa: E402


def _case(N, K, r, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.02).to(dtype)
    return w, torch.randn(r, K, generator=g) * 0.05, torch.randn(N, r, generator=g) * 0.05


def _spacing(x, dtype):
    """distance between neighbouring values of `dtype` at magnitude |x| (f64 in, f64 out)"""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("N,K,r", [(256, 256, 4), (512, 688, 13), (1024, 1024, 8)])
def test_rule_against_merge_lora(N, K, r, dtype):
    """The rule is not bit-identical to the host merge (f32 `b @ a` in the BLAS order, rounded before the add): in the 16-bit
    dtypes at most 1e-3 of the elements may differ (the host path alone: <= 2.6e-4), and every element obeys
    |diff| <= spacing(dtype, max(|a|, |b|)) + 2^-21 (|w| + s |B| |A|)  (the f32 term was measured at 3.8 * 2^-24)."""
    from anyref_amd.lora import merge_rule
    s = 16.0 / r
    w, A, B = _case(N, K, r, dtype, seed=N + K + r)
    rule = merge_rule(w, A, B, s).double()
    host = (w.float() + (B @ A) * s).to(dtype).double()
    diff = (rule - host).abs()
    share = (diff != 0).double().mean().item()
    bound = _spacing(torch.maximum(rule.abs(), host.abs()), dtype) + 2.0 ** -21 * (w.double().abs() + s * (B.double().abs() @ A.double().abs()))
    print(f"{dtype} {N}x{K} r={r}: share differing {share:.2e}, max diff {diff.max().item():.3e}")
    if dtype != torch.float32:
        assert share <= 1e-3
    assert bool((diff <= bound).all())


def test_rule_identities():
    from anyref_amd.lora import merge_rule
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        w, A, B = _case(64, 96, 5, dtype, seed=1)
        w[0, 0] = -0.0
        assert torch.equal(merge_rule(w, None, None, 2.0).view(torch.int32), w.float().view(torch.int32))     # r = 0
        assert torch.equal(merge_rule(w, A[:0], B[:, :0], 2.0).view(torch.int32), w.float().view(torch.int32))
        x = merge_rule(w, A, B, 2.0)
        assert torch.equal(x.to(dtype).float(), x)                      # m is held exactly by d_in
        # the rule reads the BASE, never the current weights: X, then Y, then X is X
        _, A2, B2 = _case(64, 96, 3, dtype, seed=2)
        y = merge_rule(w, A2, B2, 1.5)
        assert not torch.equal(x, y) and torch.equal(merge_rule(w, A, B, 2.0), x)
        # the order of j is part of the rule: the explicit chain, not a matmul
        acc = torch.zeros(64, 96, dtype=torch.float64)
        for j in range(5):
            acc = acc + B[:, j:j + 1].double() * A[j:j + 1].double()
        want = (acc * 2.0 + w.double()).float().to(dtype).float()
        assert torch.equal(x, want)
    # scaling is the f32 the C entry takes
    w, A, B = _case(32, 40, 4, torch.float32, seed=3)
    s32 = float(torch.tensor(16.0 / 13.0, dtype=torch.float32))
    assert torch.equal(merge_rule(w, A, B, 16.0 / 13.0), merge_rule(w, A, B, s32))
    # fan_in_fan_out: the adapter holds the transposed pair, delta = (b @ a).T as in merge_lora
    a_t, b_t = torch.randn(4, 32) * 0.05, torch.randn(40, 4) * 0.05
    got = merge_rule(w, a_t, b_t, 2.0, fan_in_fan_out=True)
    assert torch.equal(got, merge_rule(w, b_t.t().contiguous(), a_t.t().contiguous(), 2.0))
    assert torch.allclose(got, w + 2.0 * (b_t @ a_t).t(), atol=1e-6)
    with pytest.raises(ValueError, match="do not match"):
        merge_rule(w, A[:, :8], B, 2.0)


def test_read_adapter(tmp_path):
    from anyref_amd.checkpoint import check_adapter_shapes, merge_lora, read_adapter
    cfg = config_tiny()
    sd = synth_state_dict(cfg, seed=5, scale=0.05)
    d, want = _write_adapter(str(tmp_path), cfg, sd, torch.Generator().manual_seed(9))
    pairs, saved, scaling, fifo = read_adapter(d)
    assert scaling == 4.0 and fifo is False
    assert sorted(pairs) == sorted(f"model.layers.{i}.self_attn.{p}" for i in range(cfg.llm.layers) for p in ("q_proj", "v_proj"))
    a, b = pairs["model.layers.0.self_attn.q_proj"]
    assert a.shape == (4, cfg.llm.dim) and b.shape == (cfg.llm.dim, 4)
    assert sorted(saved) == sorted(k for k in want if "proj" not in k)            # keys under the reference's names
    # merge_lora still merges as before, through the parser
    sd2 = {k: v.half() for k, v in sd.items()}
    from anyref_amd.checkpoint import resize_token_rows
    resize_token_rows(sd2, cfg.llm.vocab + 7, seed=0)
    assert merge_lora(sd2, d) == {"lora_pairs": 2 * cfg.llm.layers, "modules_to_save": 6}
    for k, v in want.items():
        assert torch.equal(sd2[k].float(), v.float()), k
    # built shapes: the vocabulary the adapter was trained with (vocab + 7) against a model built without the resize
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    with pytest.raises(ValueError, match=rf"vocabulary of {cfg.llm.vocab + 7}.*built for {cfg.llm.vocab}"):
        check_adapter_shapes(pairs, saved, shapes, fifo)
    shapes["model.embed_tokens.weight"] = shapes["lm_head.weight"] = (cfg.llm.vocab + 7, cfg.llm.dim)
    check_adapter_shapes(pairs, saved, shapes, fifo)
    bad = dict(shapes)
    bad["model.layers.0.self_attn.q_proj.weight"] = (cfg.llm.dim, cfg.llm.dim + 8)
    with pytest.raises(ValueError, match="q_proj: the LoRA pair makes"):
        check_adapter_shapes(pairs, saved, bad, fifo)
    # a target absent from the base
    with pytest.raises(KeyError, match="which the base checkpoint does not have"):
        read_adapter(d, base_names={k for k in sd if "layers.1.self_attn.v_proj" not in k})
    # peft key forms, unpaired tensors, wrong rank
    e = str(tmp_path / "forms")
    os.makedirs(e)
    json.dump(dict(r=2, lora_alpha=4, fan_in_fan_out=True), open(os.path.join(e, "adapter_config.json"), "w"))
    A, Bm = torch.randn(2, 5), torch.randn(3, 2)
    torch.save({"base_model.model.m.lora_A.default.weight": A, "base_model.model.m.lora_B.default.weight": Bm,
                "base_model.model.head.original_module.weight": torch.zeros(1),
                "base_model.model.head.modules_to_save.default.weight": torch.full((2,), 7.0)}, os.path.join(e, "adapter_model.bin"))
    pairs, saved, scaling, fifo = read_adapter(e)
    assert list(pairs) == ["m"] and list(saved) == ["head.weight"] and scaling == 2.0 and fifo is True
    torch.save({"base_model.model.m.lora_A.weight": A}, os.path.join(e, "adapter_model.bin"))
    with pytest.raises(ValueError, match="unpaired"):
        read_adapter(e)
    torch.save({"base_model.model.m.lora_A.weight": torch.zeros(3, 5), "base_model.model.m.lora_B.weight": torch.zeros(3, 3)},
               os.path.join(e, "adapter_model.bin"))
    with pytest.raises(ValueError, match="LoRA rank 3 / 3 != r = 2"):
        read_adapter(e)
    torch.save({"base_model.model.m.lora_embedding_A": A}, os.path.join(e, "adapter_model.bin"))
    with pytest.raises(ValueError, match="unsupported adapter tensor"):
        read_adapter(e)


def test_adapter_entries_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from anyref_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "anyref_hip.h")).read(), flags=re.S)
    ops = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "anyref_hip_ops.h")).read(), flags=re.S)
    for name, txt in (("anyref_adapter_reserve", hdr), ("anyref_adapter_apply", hdr), ("anyref_update_weight", hdr),
                      ("anyref_adapter_stats", hdr), ("anyref_op_lora_merge", ops)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, f"{name} is not declared"
        assert name in _lib.SYMBOLS, f"{name} is not in the ctypes table"
        res, args = _lib.SYMBOLS[name]
        assert res is _lib._I
        assert len(args) == len(m.group(1).split(",")), f"{name}: the ctypes table and the header disagree on the argument count"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    # anyref_lora_pair: the ctypes struct lists the header's fields in the header's order
    body = hdr[hdr.index("typedef struct anyref_lora_pair {"): hdr.index("} anyref_lora_pair;")].split("{", 1)[1]
    names = [d.strip().split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.LoraPair._fields_]
    # the projection bits are the header's
    from anyref_amd.lora import TARGET_BITS
    for proj, macro in (("q_proj", "Q"), ("k_proj", "K"), ("v_proj", "V"), ("o_proj", "O"), ("gate_proj", "GATE"),
                        ("up_proj", "UP"), ("down_proj", "DOWN")):
        assert int(re.search(r"#define ANYREF_LORA_%s (\d+)u" % macro, hdr).group(1)) == TARGET_BITS[proj]
    assert re.search(r"#define ANYREF_ABI_VERSION 2\b", hdr)                      # no bump, as for sessions and drafts
    assert "lora.hip" in open(os.path.join(ROOT, "anyref_amd", "csrc", "Makefile")).read()


def test_adapters_argument_and_state_rules_without_a_gpu(tmp_path):
    from anyref_amd.lora import parse_targets, target_bit
    from anyref_amd.model import AnyRefForCausalLM
    from anyref_amd.peft_compat import PeftModel
    assert parse_targets(None) == 0 and parse_targets("qv") == 5
    assert parse_targets(["q_proj", "v_proj"]) == 5 and parse_targets(("down_proj", "gate_proj", "o_proj")) == 64 + 16 + 8
    for bad in ("q", "all", ["q_proj", "w_proj"], []):
        with pytest.raises(ValueError):
            parse_targets(bad)
    assert target_bit("model.layers.11.self_attn.v_proj.weight") == 4 and target_bit("model.layers.0.mlp.up_proj.weight") == 32
    assert target_bit("lm_head.weight") == 0 and target_bit("model.layers.0.self_attn.v_proj.bias") == 0
    # the kwarg on the constructor (and through it from_state_dict / from_pretrained); default: today's behaviour
    plain = AnyRefForCausalLM(config_tiny(), defer=True)
    resv = AnyRefForCausalLM(config_tiny(), defer=True, adapters="qv")
    assert plain.adapter_targets == 0 and resv.adapter_targets == 5 and resv.active_adapter is None
    with pytest.raises(ValueError):
        AnyRefForCausalLM(config_tiny(), defer=True, adapters="kv")
    for name in ("load_adapter", "set_adapter", "adapter_stats"):
        assert callable(getattr(AnyRefForCausalLM, name))
    # merge_and_unload, case 2: a model that is not built merges on the host as ever, reservation or not
    cfg = config_tiny()
    sd = synth_state_dict(cfg, seed=5, scale=0.05)
    d, want = _write_adapter(str(tmp_path), cfg, sd, torch.Generator().manual_seed(9))
    from anyref_amd.checkpoint import resize_token_rows
    for m in (plain, resv):
        m.load_state_dict({k: v.half() for k, v in sd.items()})
        resize_token_rows(m.host_state_dict(), cfg.llm.vocab + 7, seed=0)
        out = PeftModel.from_pretrained(m, d).merge_and_unload()
        assert out is m and m.h is None and m.adapter_stats == {"lora_pairs": 2 * cfg.llm.layers, "modules_to_save": 6}
        assert torch.equal(m.host_state_dict()["model.layers.0.self_attn.q_proj.weight"].float(),
                           want["model.layers.0.self_attn.q_proj.weight"].float())

    # cases 1 and 3 on a stand-in for a built model (the handle is only looked at, never called)
    class Built:
        h = object()
        calls = []

        def __init__(self, targets):
            self.adapter_targets = targets

        def load_adapter(self, d):
            self.calls.append(("load", d))
            return "name"

        def set_adapter(self, n):
            self.calls.append(("set", n))

        def merge_adapter(self, d):
            return AnyRefForCausalLM.merge_adapter(self, d)

        _host_sd = None

    b = Built(5)
    assert PeftModel.from_pretrained(b, "some/dir").merge_and_unload() is b
    assert b.calls == [("load", "some/dir"), ("set", "name")]
    with pytest.raises(RuntimeError, match="before .cuda"):
        PeftModel.from_pretrained(Built(0), "some/dir").merge_and_unload()
