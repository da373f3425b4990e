"""Image sessions without a GPU: the host rules of anyref_amd/session.py against known answers, and the three C entries in
the header, the ctypes table and the built library."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from anyref_amd.config import IMAGE_TOKEN_INDEX as IMG  # noqa: E402
from anyref_amd.session import check_prefix, cut_rows, has_prefix  # noqa: E402

PREFIX = [1, 17, 18, 19, IMG]


def test_prefix_must_end_with_its_only_placeholder():
    assert check_prefix(PREFIX) == PREFIX
    assert check_prefix(tuple(PREFIX)) == PREFIX
    assert check_prefix([IMG]) == [IMG]
    with pytest.raises(ValueError, match="no image placeholder"):
        check_prefix([1, 17, 18])
    with pytest.raises(ValueError, match="no image placeholder"):
        check_prefix([])
    with pytest.raises(ValueError, match="2 image placeholders"):
        check_prefix([1, IMG, 18, IMG])
    with pytest.raises(ValueError, match="END"):
        check_prefix([1, IMG, 18])


def test_prefix_detection():
    assert has_prefix(PREFIX + [40, 41], PREFIX)
    assert has_prefix(PREFIX, PREFIX)
    assert not has_prefix(PREFIX[:-1], PREFIX)                   # shorter than the prefix
    assert not has_prefix([1, 17, 18, 20, IMG, 40], PREFIX)      # another system prompt
    assert not has_prefix([40] + PREFIX, PREFIX)                 # the prefix, but not at the start


def test_full_prompts_are_cut_behind_the_placeholder_and_suffixes_pass():
    rows = [PREFIX + [40, 41, 42], [50], PREFIX + [60], [1, 17, 18, 19]]   # full, suffix, full, a suffix that looks like the prefix's text
    assert cut_rows(rows, PREFIX) == [[40, 41, 42], [50], [60], [1, 17, 18, 19]]
    # other placeholders (audio / image-ref rows: negative ids) belong to the suffix and stay where they are
    assert cut_rows([PREFIX + [40, -300, -300, 41]], PREFIX) == [[40, -300, -300, 41]]
    assert cut_rows([[40, -400]], PREFIX) == [[40, -400]]


def test_a_row_with_another_prefix_raises_and_names_the_row():
    with pytest.raises(ValueError, match="row 1 does not begin with the session's prefix"):
        cut_rows([PREFIX + [40], [1, 17, 99, 19, IMG, 40]], PREFIX)
    with pytest.raises(ValueError, match="row 0 does not begin"):
        cut_rows([[1, IMG, 17, 18, 19, 40]], PREFIX)             # the image somewhere else
    with pytest.raises(ValueError, match="row 2: 2 image placeholders"):
        cut_rows([[40], [41], PREFIX + [40, IMG]], PREFIX)
    with pytest.raises(ValueError, match="row 0: nothing follows"):
        cut_rows([PREFIX], PREFIX)
    with pytest.raises(ValueError, match="row 1: nothing follows"):
        cut_rows([[40], []], PREFIX)


def _build():
    import __graft_entry__ as g
    g.build()


def test_session_entries_are_declared_bound_and_exported():
    """as tests/test_cpu_host.py checks every symbol: the four new ones, by name"""
    _build()
    from anyref_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "anyref_hip.h")).read(), flags=re.S)
    ops = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "anyref_hip_ops.h")).read(), flags=re.S)
    for name, txt in (("anyref_session_open", hdr), ("anyref_session_generate", hdr), ("anyref_session_close", hdr),
                      ("anyref_op_kv_broadcast", ops)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, f"{name} is not declared"
        assert name in _lib.SYMBOLS, f"{name} is not in the ctypes table"
        res, args = _lib.SYMBOLS[name]
        assert res is _lib._I
        assert len(args) == len(m.group(1).split(",")), f"{name}: the ctypes table and the header disagree on the argument count"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    # the 64-bit capacity of out_masks sits where the header puts it
    decl = re.search(r"anyref_session_generate\s*\(([^;]*)\)\s*;", hdr).group(1).split(",")
    at = [i for i, a in enumerate(decl) if "out_masks_cap" in a]
    assert at and _lib.SYMBOLS["anyref_session_generate"][1][at[0]] is _lib._L


def test_python_surface_exists_without_a_gpu():
    from anyref_amd.model import AnyRefForCausalLM, ImageSession
    assert callable(AnyRefForCausalLM.image_session)
    for name in ("generate", "close", "__enter__", "__exit__"):
        assert hasattr(ImageSession, name)
