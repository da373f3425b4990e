"""SAM's spatial prompts on the CPU: the rule (anyref_amd/prompts.py) against the reference's own PromptEncoder / MaskDecoder
outputs (tests/golden/sam_prompts.npz, made by tests/golden/make_golden_prompts.py), the oracle's decoder on the rule's
output, the output selection, the coordinate transform, and the new symbols of the C surface."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prompts as gp  # noqa: E402  (config / input helpers only; touches the reference only in make())
from anyref_amd import prompts as P  # noqa: E402
from anyref_amd.synth import synth_state_dict, synth_prompt_weights, SAM_PREFIX  # noqa: E402
from oracle import anyref_oracle as O  # noqa: E402

FX = np.load(os.path.join(HERE, "golden", "sam_prompts.npz"))
SEED = int(FX["seed"])
DEC_TOL = 2e-4      # the project's decoder figure (tests/test_gpu_stages.py), x max(1, max |ref|)
# the reference computes in f32, the rule in float64: 64 f32 roundings of an O(1) value cover the PE argument (2 pi x a sum
# of two products of |G| <~ 4) and the three small convolutions
F32_TOL = 64 * 2.0 ** -24


@pytest.fixture(scope="module")
def world():
    sd = gp.prompt_weights(SEED)
    emb, sets = gp.prompt_inputs(SEED)
    wsum = gp.checksum(sd, SAM_PREFIX + "prompt_encoder.") + gp.checksum(sd, SAM_PREFIX + "mask_decoder.")
    assert abs(wsum - float(FX["wsum"])) <= 1e-9 * float(FX["wsum"]), "the weight generators drifted from the fixture's"
    assert abs(gp.insum(emb, sets) - float(FX["insum"])) <= 1e-9 * float(FX["insum"]), "the input generator drifted"
    return gp.cfg(), sd, emb, sets


def close(got, ref, tol, what):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = (got - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f"    {what}: err/scale {err / scale:.3e} (tol {tol:g})")
    assert np.isfinite(err) and err <= tol * scale, f"{what}: max abs err {err:.3e}, scale {scale:.3e}, tol {tol}"


def test_synth_prompt_weights_leave_the_state_dict_alone():
    cfg = gp.cfg()
    a, b = synth_state_dict(cfg, seed=SEED, scale=0.05), synth_prompt_weights(cfg, seed=SEED)
    assert not set(a) & set(b)
    assert sorted(k[len(P.PE_PREFIX):] for k in b) == sorted(P.SPATIAL_NAMES)
    assert b[P.PE_PREFIX + "mask_downscaling.0.weight"].shape == (4, 1, 2, 2)
    assert b[P.PE_PREFIX + "mask_downscaling.3.weight"].shape == (16, 4, 2, 2)
    assert b[P.PE_PREFIX + "mask_downscaling.6.weight"].shape == (cfg.sam.out_chans, 16, 1, 1)


@pytest.mark.parametrize("name", gp.SETS)
def test_encode_matches_the_reference(world, name):
    cfg, sd, _, sets = world
    sparse, dense = P.encode(sd, cfg, **sets[name])
    ns = {"points": 3, "box_mask": 2, "all": 5, "text": 1}[name]        # 2 points + pad; 2 corners; 2 + 2 + text; text
    assert sparse.shape == (3, ns, cfg.sam.out_chans) and sparse.dtype == torch.float64
    close(sparse, FX[f"{name}_sparse"], F32_TOL, f"{name}: sparse")
    close(dense[:, ::4, ::2, ::2], FX[f"{name}_dense"], F32_TOL, f"{name}: dense")


@pytest.mark.parametrize("name", gp.SETS)
def test_oracle_decoder_on_the_rule(world, name):
    cfg, sd, emb, sets = world
    sparse, dense = P.encode(sd, cfg, **sets[name])
    with torch.no_grad():
        m4, iou = O.mask_decoder_predict(sd, cfg, emb, O.dense_pe(sd, cfg), sparse.float(), dense.float())
    close(iou, FX[f"{name}_iou"], DEC_TOL, f"{name}: iou")
    tokens, best = P.pick(iou, True)
    assert best.tolist() == FX[f"{name}_best"].tolist()
    if name == "all":
        close(m4[:, :, ::2, ::2], FX["all_masks4"], DEC_TOL, "all: predict_masks")
        close(m4[:, tokens][:, :, ::2, ::2], FX["all_multi"], DEC_TOL, "all: multimask_output=True")
        close(iou[:, tokens], FX["all_iou_multi"], DEC_TOL, "all: multimask iou")
        post = O.postprocess_masks(cfg, m4[:, tokens], *gp.POST_SIZES)
        close(post[:, :, ::8, ::8], FX["all_post"], DEC_TOL, "all: postprocess_masks")


def test_pick():
    iou = torch.tensor([[0.9, 0.1, 0.7, 0.3], [0.0, 0.2, 0.1, 0.6]])
    tok, best = P.pick(iou, False)
    assert (tok.start, tok.stop) == (0, 1) and best.tolist() == [0, 0]
    tok, best = P.pick(iou, True)
    assert (tok.start, tok.stop) == (1, 4) and best.tolist() == [1, 2]        # token 0's 0.9 does not count


def test_to_input_frame():
    # 301 x 437 (h x w) resized to 150 x 224 -- x by 224 / 437, y by 150 / 301
    got = P.to_input_frame([[437.0, 301.0], [100.0, 50.0], [0.0, 0.0]], (301, 437), (150, 224))
    want = torch.tensor([[224.0, 150.0], [100.0 * (224 / 437), 50.0 * (150 / 301)], [0.0, 0.0]], dtype=torch.float64)
    assert got.dtype == torch.float32 and torch.equal(got, want.to(torch.float32))
    # a portrait image: the long side is the height
    got = P.to_input_frame([[10.0, 20.0]], (640, 480), (1024, 768))
    assert torch.equal(got, torch.tensor([[16.0, 32.0]]))
    # a box goes through as its two corners
    got = P.to_input_frame(torch.tensor([4.0, 8.0, 40.0, 80.0]).reshape(2, 2), (100, 200), (50, 100)).reshape(4)
    assert got.tolist() == [2.0, 4.0, 20.0, 40.0]


NEW = ("anyref_prompt_reserve", "anyref_mask_decode_prompted", "anyref_refine_masks", "anyref_refine_embedding",
       "anyref_op_prompt_tokens", "anyref_op_mask_prompt_embed")


def test_new_symbols_everywhere():
    from anyref_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "anyref_hip.h")).read() + open(os.path.join(ROOT, "include", "anyref_hip_ops.h")).read()
    for s in NEW:
        assert re.search(r"\bint %s\(" % s, hdr), f"{s} is not declared in the headers"
        assert s in _lib.SYMBOLS, f"{s} is not in the ctypes table"
    assert "typedef struct anyref_spatial_prompts" in hdr
    assert [f[0] for f in _lib.SpatialPrompts._fields_] == ["points", "labels", "n_points", "boxes", "mask_input", "multimask"]
    assert os.path.exists(_lib.LIB_PATH), "build the backend first (__graft_entry__.build())"
    lib = C.CDLL(_lib.LIB_PATH)       # dlopen only: no device is touched
    for s in NEW:
        assert hasattr(lib, s), f"{s} is not exported by the built library"


def test_python_surface_builds_a_deferred_handle_first():
    """every new method that talks to the handle is in the list that triggers a deferred build (from_pretrained's flow)"""
    from anyref_amd import model as M
    for name in ("set_spatial_prompts", "refine", "refine_embedding", "mask_decode"):
        assert name in M._NEEDS_HANDLE and callable(getattr(M.AnyRefForCausalLM, name)), name
    assert callable(M.ImageSession.refine)
