"""The token-score rule (anyref_amd/scores.py) held to torch's own log_softmax / topk and to its stated edge
cases, and the interface that carries it: the three symbols in the library and their declarations in the two headers.
No GPU: the library is only opened for its symbol table."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from anyref_amd.scores import token_scores_rows, token_scores_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("N", [2, 5, 1000, 32007])
@pytest.mark.parametrize("scale", [0.05, 1.0, 30.0])
def test_rule_agrees_with_log_softmax_and_topk(N, scale):
    g = torch.Generator().manual_seed(N)
    x = torch.randn(6, N, generator=g) * scale
    ids, lp, gap = token_scores_rows(x)
    ref_lp = torch.log_softmax(x.double(), -1)
    top = torch.topk(x, 2, dim=-1)
    assert ids.tolist() == torch.argmax(x, -1).tolist()
    for r in range(x.shape[0]):
        want = ref_lp[r, ids[r]].item()
        assert abs(lp[r] - want) <= 1e-12 * max(1.0, abs(want)), (r, lp[r], want)
        assert gap[r] == (top.values[r, 0] - top.values[r, 1]).item(), "the f32 subtraction of the two greatest values"
        assert gap.dtype == np.float32 and lp[r] <= 0.0 and gap[r] >= 0.0


def test_tie_gives_the_first_index_and_gap_zero():
    x = torch.tensor([0.5, 2.0, -1.0, 2.0, 2.0, 0.0])
    i, lp, gap = token_scores_rule(x)
    assert (i, gap) == (1, 0.0)
    assert abs(lp - torch.log_softmax(x.double(), -1)[1].item()) < 1e-15
    assert token_scores_rule(np.array([3.0, 3.0], dtype=np.float32))[::2] == (0, 0.0)


def test_nan_row():
    x = torch.tensor([0.5, INF, NAN, 1.0, NAN])
    i, lp, gap = token_scores_rule(x)
    assert i == 2 == int(torch.argmax(x)), "NaN counts as the greatest value, the first one is the id"
    assert math.isnan(lp) and math.isnan(gap)
    i, lp, gap = token_scores_rule(torch.full((7,), NAN))
    assert i == 0 and math.isnan(lp) and math.isnan(gap)


def test_minus_inf_entries_add_nothing():
    x = torch.tensor([-INF, 1.0, -INF, 3.0, 2.0, -INF])
    i, lp, gap = token_scores_rule(x)
    j, lp2, gap2 = token_scores_rule(torch.tensor([1.0, 3.0, 2.0]))
    assert (i, j) == (3, 1) and lp == lp2 and gap == gap2 == 1.0
    # one finite entry: it holds all the mass, the runner-up is -inf
    i, lp, gap = token_scores_rule(torch.tensor([-INF, -INF, 0.25]))
    assert (i, lp, gap) == (2, 0.0, INF)
    # what IEEE gives for the formula stands: a row of -inf is m - m = NaN
    i, lp, gap = token_scores_rule(torch.full((4,), -INF))
    assert i == 0 and math.isnan(lp) and math.isnan(gap)
    i, lp, gap = token_scores_rule(torch.tensor([0.0, INF, 1.0]))
    assert i == 1 and math.isnan(lp) and gap == INF


@pytest.mark.parametrize("N", [2, 5, 32007])
def test_all_equal_row(N):
    i, lp, gap = token_scores_rule(torch.full((N,), -3.25))
    assert i == 0 and gap == 0.0 and abs(lp + math.log(N)) <= 1e-12


def test_no_overflow_at_large_logits():
    x = torch.full((1000,), -1e4)
    x[17] = 1e4
    assert token_scores_rule(x) == (17, 0.0, 2e4)


def test_refused_inputs():
    with pytest.raises(ValueError):
        token_scores_rule(torch.tensor([1.0]))
    with pytest.raises(ValueError):
        token_scores_rule(torch.zeros(2, 3))
    with pytest.raises(TypeError):
        token_scores_rule(torch.zeros(4, dtype=torch.float64))


NAMES = ("anyref_set_token_scores", "anyref_token_scores", "anyref_op_token_scores")


def test_library_exports_the_symbols():
    from anyref_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the backend first (__graft_entry__.build())"
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SYMBOLS, f"{name} is not bound in anyref_amd/_lib.py"
        getattr(lib, name)          # AttributeError: not exported


def test_headers_declare_them():
    api = open(os.path.join(ROOT, "include", "anyref_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "anyref_hip_ops.h")).read()
    assert re.search(r"^int anyref_set_token_scores\(anyref_handle\* h, int on\);", api, re.M)
    assert re.search(r"^int anyref_token_scores\(anyref_handle\* h, int B, int n_cap, float\* logprob, float\* gap, int32_t\* n\);",
                     api, re.M)
    assert re.search(r"^int anyref_op_token_scores\(void\* stream, const float\* logits, int M, int N, int ldx, "
                     r"const int32_t\* dst, float\* logprob,\s+float\* gap, int64_t\* id\);", ops, re.M)
