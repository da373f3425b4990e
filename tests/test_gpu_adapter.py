"""Adapter hot-swap on a live handle (`adapters="qv"`, `load_adapter`, `set_adapter`): a reserving handle
switched to an adapter computes, bit for bit, what a fresh handle built from the rule's merged state dict computes -- in every
weight format -- and agrees with the CPU oracle on those weights; switching on, between and off adapters never drifts; the
captured decode graphs replay the new weights; an open image session ends; a refused apply changes nothing; a handle that
reserves nothing is as it always was."""
import copy
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

from anyref_amd import _lib  # noqa: E402
from anyref_amd.checkpoint import read_adapter  # noqa: E402
from anyref_amd.config import config_tiny  # noqa: E402
from anyref_amd.lora import merged_state_dict  # noqa: E402
from anyref_amd.synth import synth_state_dict  # noqa: E402
from oracle import anyref_oracle as O  # noqa: E402
from test_cpu_checkpoint import _write_adapter  # noqa: E402
from test_gpu_e2e import make_inputs, rig_seg  # noqa: E402

NEW = 6
SIZES, HH, WW = [(224, 180)], [120], [97]


class Rig:
    """one base model, two adapters on disk (Y without text_hidden_fcs), one prompt; built once for the module"""

    def __init__(self, tmp):
        self.cfg = config_tiny()                              # 2 LLaMA layers
        wcfg = config_tiny()
        wcfg.llm.vocab = self.cfg.llm.vocab - 7               # _write_adapter saves embed_tokens / lm_head with vocab + 7 rows
        self.sd = synth_state_dict(self.cfg, seed=3, scale=0.05)
        self.clip, self.sam, self.ids = make_inputs(self.cfg, 1, seed=4)
        rig_seg(self.cfg, self.sd, self.clip, self.sam, self.ids, SIZES, (HH, WW))
        self.dirs = {}
        for name, seed in (("X", 21), ("Y", 22)):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            self.dirs[name], _ = _write_adapter(d, wcfg, self.sd, torch.Generator().manual_seed(seed))
        p = os.path.join(self.dirs["Y"], "adapter_model.bin")
        ad = torch.load(p)
        torch.save({k: v for k, v in ad.items() if "text_hidden_fcs" not in k}, p)
        self.base_seg = self.cfg.seg_token_idx                                      # the [SEG] id the BASE weights emit
        self.n_rows = len(self.ids[0]) - 1 + self.cfg.clip.n_patches + NEW - 1     # hidden rows a call writes

    def base_sd(self, dtype=None):
        return {k: (v.to(dtype) if dtype else v) for k, v in self.sd.items()}

    def merged_sd(self, name, dtype=None):
        """the state dict a fresh handle needs to hold what set_adapter(name) leaves (None: the base)"""
        sd = self.base_sd(dtype)
        if name is None:
            return sd
        pairs, saved, scaling, fifo = read_adapter(self.dirs[name])
        return merged_state_dict(sd, pairs, saved, scaling, fifo)

    def build(self, mode, sd, adapters=None, cfg=None):
        from anyref_amd.model import AnyRefForCausalLM
        m = AnyRefForCausalLM.from_state_dict(copy.deepcopy(cfg or self.cfg), {k: v.cuda() for k, v in sd.items()}, mode=mode,
                                              max_batch=1, max_seg=8, adapters=adapters)
        m.config.eos_token_id = None
        return m

    def seg_of(self, m):
        """the id this handle emits one before its last token: named as [SEG], its weights make a mask (rig_seg's trick)"""
        return self.gen(m)["ids"][-2]

    def gen(self, m, seg=None):
        if seg is not None:
            m.set_seg_token_idx(seg)
        (out_ids, masks, _), ex = m.generate(self.clip, self.ids[0][None], self.sam, SIZES, HH, WW, max_new_tokens=NEW,
                                             _return_extras=True)
        return dict(ids=out_ids[0].cpu().tolist(), masks=[x.cpu() for x in (masks or [])],
                    hidden=ex["hidden"][0, : self.n_rows].cpu())


def same(a, b):
    return (a["ids"] == b["ids"] and len(a["masks"]) == len(b["masks"]) and
            all(torch.equal(x, y) for x, y in zip(a["masks"], b["masks"])) and torch.equal(a["hidden"], b["hidden"]))


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    return Rig(str(tmp_path_factory.mktemp("adapters")))


def test_parity_against_the_oracle_and_a_fresh_handle(rig):
    wX = rig.merged_sd("X")
    cfg = copy.deepcopy(rig.cfg)
    rig_seg(cfg, wX, rig.clip, rig.sam, rig.ids, SIZES, (HH, WW))      # the [SEG] id the merged weights emit
    with torch.no_grad():
        ref = O.anyref_generate(wX, cfg, rig.clip, rig.ids, rig.sam, SIZES, HH, WW, max_new_tokens=NEW, eos=False)
    fresh = rig.build("parity", wX, cfg=cfg)
    f1, f2 = rig.gen(fresh), rig.gen(fresh)
    assert same(f1, f2), "two runs of one handle are not bit-identical: nothing below can be"
    assert f1["masks"] and f1["masks"][0].numel()
    m = rig.build("parity", rig.base_sd(), adapters="qv", cfg=cfg)
    m.set_adapter(m.load_adapter(rig.dirs["X"]))
    got = rig.gen(m)
    assert got["ids"] == ref["output_ids"][0].tolist()
    assert ref["pred_masks"] is not None and got["masks"][0].shape == ref["pred_masks"][0].shape
    assert (got["masks"][0] - ref["pred_masks"][0]).abs().max().item() <= 1e-3
    assert same(got, f1)
    assert m.inexact_weights == 0 and m.active_adapter == "adapter"     # default name: the directory's


@pytest.mark.parametrize("mode,dtype", [("perf", None), ("perf_f16", torch.float16), ("perf_int4w", None), ("perf_fp8w", None),
                                        ("parity16", torch.bfloat16)])
def test_switched_handle_equals_fresh_handle(rig, mode, dtype):
    """the packed weights are the same bits by construction, in every storage format; `dtype`: what the base is handed over in"""
    fresh = rig.build(mode, rig.merged_sd("X", dtype))
    seg = rig.seg_of(fresh)
    f1 = rig.gen(fresh, seg)
    assert same(f1, rig.gen(fresh)) and f1["masks"] and f1["masks"][0].numel()
    n_fresh = fresh.inexact_weights
    del fresh
    m = rig.build(mode, rig.base_sd(dtype), adapters="qv")
    m.set_adapter(m.load_adapter(rig.dirs["X"]))
    assert same(rig.gen(m, seg), f1)
    assert m.inexact_weights == n_fresh                      # the counters of the merge feed anyref_inexact_weights


def test_x_y_none_x_without_drift_and_graph_replay(rig):
    mode = "perf"
    m = rig.build(mode, rig.base_sd(), adapters=["q_proj", "v_proj"])
    m.set_graphs(True)
    base0 = rig.gen(m)                                       # captures the decode graph on the base weights
    m.load_adapter(rig.dirs["X"], name="X")
    m.load_adapter(rig.dirs["Y"], name="Y")
    layers = rig.cfg.llm.layers
    assert m.adapter_stats()["targets_reserved"] == 2 * layers and m.adapter_stats()["pairs_active"] == 0
    m.set_adapter("X")
    st = m.adapter_stats()
    assert st["pairs_active"] == 2 * layers and st["last_apply_ms"] > 0 and st["active_adapter"] == "X"
    fx = rig.build(mode, rig.merged_sd("X"))
    seg_x = rig.seg_of(fx)
    x1 = rig.gen(m, seg_x)                                   # graph replay on the new weights
    assert same(x1, rig.gen(fx, seg_x)) and x1["masks"]
    del fx
    assert x1["ids"] != base0["ids"] or not torch.equal(x1["hidden"], base0["hidden"])
    m.set_adapter("Y")                                       # Y carries no text_hidden_fcs: the built ones come back
    fy = rig.build(mode, rig.merged_sd("Y"))
    seg_y = rig.seg_of(fy)
    y_ref = rig.gen(fy, seg_y)
    assert same(rig.gen(m, seg_y), y_ref) and y_ref["masks"]
    del fy
    m.set_adapter(None)
    assert m.adapter_stats()["pairs_active"] == 0 and m.active_adapter is None
    never = rig.build(mode, rig.base_sd())
    n0 = rig.gen(never)
    assert same(rig.gen(m, rig.base_seg), n0) and same(base0, n0) and n0["masks"]
    assert m.inexact_weights == never.inexact_weights
    m.set_adapter("X")
    assert same(rig.gen(m, seg_x), x1)                       # X -> Y -> None -> X: no drift


def test_session_ends_and_a_new_one_works(rig):
    m = rig.build("perf", rig.base_sd(), adapters="qv")
    name = m.load_adapter(rig.dirs["X"])
    ids = rig.ids[0]
    cut = 2                                                  # BOS + image placeholder
    sess = m.image_session(rig.clip[0], rig.sam[0], SIZES[0], HH[0], WW[0], ids[:cut])
    sess.generate(ids[None], max_new_tokens=NEW)
    m.set_adapter(name)
    with pytest.raises(RuntimeError, match="ended by anyref_adapter_apply"):
        sess.generate(ids[None], max_new_tokens=NEW)
    sess.close()
    plain = rig.gen(m)
    with m.image_session(rig.clip[0], rig.sam[0], SIZES[0], HH[0], WW[0], ids[:cut]) as s2:
        out_ids, masks, _ = s2.generate(ids[None], max_new_tokens=NEW)
    assert out_ids[0].cpu().tolist() == plain["ids"]


def test_refused_apply_leaves_the_weights(rig):
    m = rig.build("perf", rig.base_sd(), adapters="qv")
    m.set_adapter(m.load_adapter(rig.dirs["X"]))
    before = rig.gen(m)
    H = rig.cfg.llm.dim
    A, B = torch.randn(65, H, device="cuda"), torch.randn(H, 65, device="cuda")
    good = (torch.randn(4, H, device="cuda"), torch.randn(H, 4, device="cuda"))

    def apply(rows):
        arr = (_lib.LoraPair * len(rows))()
        keep = []
        for i, (nm, a, b, r) in enumerate(rows):
            keep.append(nm.encode())
            arr[i].weight_name, arr[i].A, arr[i].B, arr[i].r, arr[i].is_device = keep[-1], a.data_ptr(), b.data_ptr(), r, 1
        rc = m.lib.anyref_adapter_apply(m.h, None, arr, len(rows), 1.0)
        torch.cuda.synchronize()
        return rc, m.lib.anyref_last_error(m.h).decode()

    q0, v1 = "model.layers.0.self_attn.q_proj.weight", "model.layers.1.self_attn.v_proj.weight"
    # a valid pair FIRST in each list: validation must finish before anything is written
    rc, err = apply([(v1, *good, 4), (q0, A, B, 65)])
    assert rc != 0 and q0 in err and "outside 1 .. 64" in err
    rc, err = apply([(v1, *good, 4), ("model.layers.0.self_attn.k_proj.weight", *good, 4)])
    assert rc != 0 and "k_proj" in err and "not a reserved" in err
    rc, err = apply([(v1, *good, 4), (v1, *good, 4)])
    assert rc != 0 and "twice" in err
    assert same(rig.gen(m), before)
    assert m.adapter_stats()["pairs_active"] == 2 * rig.cfg.llm.layers


def test_no_reservation_is_unchanged(rig):
    plain = rig.build("perf", rig.base_sd())
    with pytest.raises(RuntimeError, match="adapters="):
        plain.load_adapter(rig.dirs["X"])
    arr = (_lib.LoraPair * 1)()
    assert plain.lib.anyref_adapter_apply(plain.h, None, arr, 0, 1.0) != 0
    assert "reserved no LoRA targets" in plain.lib.anyref_last_error(plain.h).decode()
    st = plain.adapter_stats()
    assert st["targets_reserved"] == 0 and st["pairs_active"] == 0
    resv = rig.build("perf", rig.base_sd(), adapters="qv")
    H, T = rig.cfg.llm.dim, 2 * rig.cfg.llm.layers
    # the reservation costs the retained f32 tensors and two counters per target (nothing else: no scratch outside the
    # quantised modes); the plain handle holds none of it, i.e. what it held before adapters existed
    assert resv.device_bytes - plain.device_bytes == T * H * H * 4 + T * 16
    # reserve is refused once the weights are packed
    assert plain.lib.anyref_adapter_reserve(plain.h, 5) != 0
    assert "after anyref_finalize" in plain.lib.anyref_last_error(plain.h).decode()
