"""ANYREF_MODE_PERF_F16 at the host boundary (no GPU needed): the mode code in the header and the ctypes table, the
weight-exactness query in both, and the Python mode name reaching the loud no-GPU failure like every other mode."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()


def test_perf_f16_mode_code_in_header_and_ctypes():
    from anyref_amd import _lib
    txt = open(os.path.join(ROOT, "include", "anyref_hip.h")).read()
    m = re.search(r"#define\s+ANYREF_MODE_PERF_F16\s+(\d+)", txt)
    assert m and int(m.group(1)) == 4
    assert _lib.MODE_PERF_F16 == 4
    assert _lib.ABI_VERSION == 2      # anyref_config is unchanged


def test_inexact_weights_is_declared_and_exported():
    _build()
    from anyref_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "anyref_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+anyref_inexact_weights\s*\(\s*anyref_handle\s*\*\s*h\s*,\s*int64_t\s*\*\s*out\s*\)", txt)
    assert "anyref_inexact_weights" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "anyref_inexact_weights")


def test_perf_f16_without_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _build()
    from anyref_amd.config import config_tiny
    from anyref_amd.model import AnyRefForCausalLM
    with pytest.raises(RuntimeError, match="MI355X"):
        AnyRefForCausalLM(config_tiny(), mode="perf_f16")
