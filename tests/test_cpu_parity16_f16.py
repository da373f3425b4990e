"""ANYREF_MODE_PARITY16_F16 at the host boundary (no GPU needed): the mode code in the header and the ctypes table, an
unchanged ABI version (anyref_config did not grow), the kernel-level round-trip entry declared and exported, and the Python
mode name "parity16_f16" reaching the loud no-GPU failure like every other mode."""
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


def test_parity16_f16_mode_code_in_header_and_ctypes():
    from anyref_amd import _lib
    txt = open(os.path.join(ROOT, "include", "anyref_hip.h")).read()
    m = re.search(r"#define\s+ANYREF_MODE_PARITY16_F16\s+(\d+)", txt)
    assert m and int(m.group(1)) == 5
    assert _lib.MODE_PARITY16_F16 == 5
    codes = [int(v) for v in re.findall(r"#define\s+ANYREF_MODE_\w+\s+(\d+)", txt)]
    assert sorted(codes) == list(range(6)), codes          # six modes, no code used twice
    v = re.search(r"#define\s+ANYREF_ABI_VERSION\s+(\d+)", txt)
    assert v and int(v.group(1)) == 2 and _lib.ABI_VERSION == 2      # anyref_config is unchanged


def test_split_roundtrip_entry_is_declared_and_exported():
    _build()
    from anyref_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "anyref_hip_ops.h")).read(), flags=re.S)
    assert re.search(r"int\s+anyref_op_split_roundtrip\s*\(", txt)
    assert "anyref_op_split_roundtrip" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "anyref_op_split_roundtrip")


def test_parity16_f16_without_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _build()
    from anyref_amd.config import config_tiny
    from anyref_amd.model import AnyRefForCausalLM
    with pytest.raises(RuntimeError, match="MI355X"):
        AnyRefForCausalLM(config_tiny(), mode="parity16_f16")


def test_unknown_mode_name_is_still_refused():
    from anyref_amd.config import config_tiny
    from anyref_amd.model import AnyRefForCausalLM
    with pytest.raises(KeyError):
        AnyRefForCausalLM(config_tiny(), mode="parity16_f32")
