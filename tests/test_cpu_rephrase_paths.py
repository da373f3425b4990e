"""The rephrase branch on the fast paths, what can be checked without a GPU: the library exports the new
entries and the Python layer binds them; the float64 restatement of the two passes (tests/rephrase_ref.py) agrees with the
oracle's `generate_tail`; a session applies the reference's "fewer [SEG]s than samples" rule per row."""
import ctypes as C
import os

import pytest
import torch

import rephrase_ref as R


def test_library_exports_and_python_methods():
    from anyref_amd import _lib
    from anyref_amd.model import AnyRefForCausalLM
    assert os.path.exists(_lib.LIB_PATH), "build the HIP backend first"
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("anyref_set_rephrase_paths", "anyref_op_seg_rephrase", "anyref_early_masks_done"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
    assert callable(AnyRefForCausalLM.set_rephrase_paths)
    assert isinstance(AnyRefForCausalLM.early_masks_done, property)


class _Captured(Exception):
    pass


def oracle_term(monkeypatch, attn, hidden, s0, e0, weight):
    """what oracle/anyref_oracle.py `generate_tail` itself adds to the [SEG] row (its lines for anyref.py:745-754,769), by calling
    it: a one-sample call whose [SEG] is predicted by hidden row e0 behind a prompt of s0 - 254 ids, stopped where it hands the
    rows to text_hidden_fcs.  attn [heads, S, S], hidden [S, D] float64"""
    from types import SimpleNamespace
    from oracle import anyref_oracle as O
    SEG = 7
    cfg = SimpleNamespace(rephrase_weight=weight, seg_range=lambda: (SEG, SEG))
    ids = torch.zeros(hidden.shape[0] - 254 + 1, dtype=torch.long)
    ids[e0 - 255 + 1] = SEG                                   # found at p = e0 - 255 of ids[1:]: hidden row p + 255

    def capture(w, h):
        raise _Captured(h)

    monkeypatch.setattr(O, "text_hidden_fc", capture)
    with pytest.raises(_Captured) as got:
        O.generate_tail(None, cfg, [ids], [s0 - 254], [hidden], [attn], None, None, None, None)
    return got.value.args[0][0] - hidden[e0]


@pytest.mark.parametrize("heads,hd,S,s0,e0", [(4, 64, 268, 256, 258), (5, 16, 265, 259, 260), (3, 8, 296, 277, 295)])
def test_reference_agrees_with_the_oracle(monkeypatch, heads, hd, S, s0, e0):
    """random q, K, hidden: the causal softmax matrix per head handed to the oracle's generate_tail as `attentions[-1][b]` --
    against the two passes, which see row e0 and keys [0, e0] only"""
    g = torch.Generator().manual_seed(heads * 100 + e0)
    q = torch.randn(1, S, heads, hd, generator=g, dtype=torch.float64)
    k = torch.randn(1, S, heads, hd, generator=g, dtype=torch.float64)
    hidden = torch.randn(1, S, heads * hd, generator=g, dtype=torch.float64)
    scale, weight = hd ** -0.5, 0.1
    s = torch.einsum("ihd,jhd->hij", q[0], k[0]) * scale
    s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    want = oracle_term(monkeypatch, torch.softmax(s, dim=-1), hidden[0], s0, e0, weight)
    got, bound = R.seg_rephrase(q, k, hidden, (0, e0, s0, 0), scale, weight)
    assert (got - want).abs().max().item() <= 1e-12
    assert (bound > 0).all()
    # rows the passes may not read change nothing
    q2, k2, h2 = q.clone(), k.clone(), hidden.clone()
    q2[0, :e0] = float("nan"); q2[0, e0 + 1:] = float("nan")
    k2[0, e0 + 1:] = float("nan")
    h2[0, :s0] = float("nan"); h2[0, e0:] = float("nan")
    again, _ = R.seg_rephrase(q2, k2, h2, (0, e0, s0, 0), scale, weight)
    assert torch.equal(again, got)


def test_session_rows_take_the_no_mask_rule_per_row():
    """`_result(per_row=True)`: with rephrasing, rows without a [SEG] get an empty mask tensor and the others keep theirs; the
    batched call keeps the reference's rule (one all-zero mask per sample)"""
    from anyref_amd.config import config_tiny
    from anyref_amd.model import AnyRefForCausalLM
    cfg = config_tiny()
    cfg.rephrase_weight = 0.5
    m = AnyRefForCausalLM.__new__(AnyRefForCausalLM)
    sa = lambda k, v: object.__setattr__(m, k, v)
    sa("cfg", cfg); sa("config", cfg); sa("device", torch.device("cpu")); sa("success_arity", 3)
    res = object.__getattribute__(m, "_result")
    h, w = [3, 3, 3], [2, 2, 2]
    out_ids = torch.arange(12).view(3, 4)
    lens = torch.tensor([4, 3, 4], dtype=torch.int32)
    nseg = torch.tensor([1, 0, 0], dtype=torch.int32)
    offs = torch.tensor([0, 6, 6])
    masks = torch.arange(18, dtype=torch.float32)
    _, rows, _ = res(out_ids, lens, nseg, offs, masks, h, w, per_row=True)
    assert [tuple(t.shape) for t in rows] == [(1, 3, 2), (0, 3, 2), (0, 3, 2)]
    assert torch.equal(rows[0].flatten(), masks[:6])
    _, batch, _ = res(out_ids, lens, nseg, offs, masks, h, w)
    assert all(tuple(t.shape) == (1, 3, 2) and float(t.abs().sum()) == 0.0 for t in batch)
    assert res(out_ids, lens, torch.zeros(3, dtype=torch.int32), offs, masks, h, w, per_row=True)[1] is None
