"""Proves tests/prompt_ops_ref.py without a GPU, at the very shapes tests/test_gpu_prompt_ops.py runs: for both spatial-prompt
kernels an f32 emulation in the kernel's own order lies inside the bound and every mutant lies outside; the copied rows of the
token matrix are bit for bit; every loss is exercised by at least one case; and the references agree with the rule
(anyref_amd/prompts.py) they restate."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_ops_ref as PR  # noqa: E402
import glue_ops_ref as R  # noqa: E402


@pytest.mark.parametrize("case", PR.TOKEN_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_prompt_tokens(case):
    c = PR.token_case(*case)
    emu = PR.prompt_tokens(c["out_tokens"], c["points"], c["labels"], c["boxes"], c["text"], c["gauss"], c["emb5"], c["S"],
                           emulate=True)
    n, P, box, text, C = case
    assert c["ref"].shape == (n, PR.token_rows(PR.TOKEN_N_OUT, P, box, text), C)
    R.check_bound(emu, c["ref"], c["bound"], c["mutants"], f"cpu prompt_tokens {case}")
    exact = c["bound"] == 0                       # copied rows: the emulation holds the operand's own bits
    assert exact[:, : PR.TOKEN_N_OUT].all() and (R.bits(emu)[exact] == R.bits(c["ref"].float())[exact]).all()


def test_prompt_tokens_mutants_cover_every_loss():
    seen = set()
    for case in PR.TOKEN_CASES:
        seen |= set(PR.token_losses(*case))
    assert seen == set(PR.TOKEN_LOSSES)


@pytest.mark.parametrize("case", PR.EMBED_CASES, ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_mask_prompt_embed(case):
    n, g, C, c1, c2 = case[:5]
    c = PR.embed_case(*case)
    emu = PR.mask_prompt_embed(c["mask"], c["emb"], c["W"], g, emulate=True)
    R.check_bound(emu, c["ref"], c["bound"], c["mutants"], f"cpu mask_prompt_embed {case[:5]}")


def test_mask_prompt_embed_mutants_cover_every_loss():
    seen = set()
    for case in PR.EMBED_CASES:
        seen |= set(PR.embed_case(*case)["mutants"])
    assert seen == set(PR.EMBED_LOSSES)


def test_references_restate_the_rule():
    """the two references against anyref_amd.prompts.encode on the same operands (float64 both: agreement to rounding)"""
    from types import SimpleNamespace
    from anyref_amd import prompts as P
    n, pts, box, text, C = PR.TOKEN_CASES[1]
    c = PR.token_case(n, pts, box, text, C)
    g = 5
    e = PR.embed_case(2, g, 64, 4, 16)
    cfg = SimpleNamespace(sam=SimpleNamespace(img_size=c["S"], out_chans=C, grid=g))
    pre = P.PE_PREFIX
    w = {pre + "pe_layer.positional_encoding_gaussian_matrix": c["gauss"], pre + "not_a_point_embed.weight": c["emb5"][4:5],
         pre + "no_mask_embed.weight": torch.zeros(1, C)}
    w.update({pre + f"point_embeddings.{i}.weight": c["emb5"][i:i + 1] for i in range(4)})
    sparse, _ = P.encode(w, cfg, c["points"], c["labels"], None, None, c["text"])
    assert (sparse - c["ref"][:, PR.TOKEN_N_OUT:]).abs().max() < 1e-12
    W = e["W"]
    md = pre + "mask_downscaling."
    w2 = {md + "0.weight": W["w1"], md + "0.bias": W["b1"], md + "1.weight": W["g1"], md + "1.bias": W["be1"],
          md + "3.weight": W["w2"], md + "3.bias": W["b2"], md + "4.weight": W["g2"], md + "4.bias": W["be2"],
          md + "6.weight": W["w3"], md + "6.bias": W["b3"]}
    dense = P.mask_downscaling(w2, e["mask"])                                  # [n, C, g, g]
    keys = dense.permute(0, 2, 3, 1).reshape(2, g * g, 64) + e["emb"].double()
    assert (keys - e["ref"]).abs().max() < 1e-12
