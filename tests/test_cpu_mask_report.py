"""The mask-report rule (anyref_amd/maskreport.py) held exactly to what the reference's
`calculate_stability_score`, `batched_mask_to_box` and `mask_to_rle_pytorch` returned for the recorded inputs
(tests/golden/mask_report_amg.npz, written by tests/golden/make_golden_mask_report.py), six mutants of the rule that those
inputs must tell apart, and the interface that carries it: symbols, headers, and the launcher's ledger.
No GPU: the library is only opened for its symbol table."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from anyref_amd.maskreport import mask_report_rule, pack_bits, packed_width, rle, stability, unpack

from test_cpu_glue_ops_ref import declared_launchers, ledger_problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "mask_report_amg.npz"))
SHAPES = [tuple(int(v) for v in s) for s in GOLD["shapes"]]
OFFSET = float(GOLD["offset"])


def _case(i):
    n = SHAPES[i][0]
    lens = GOLD[f"rle_lens_{i}"]
    flat = GOLD[f"rle_counts_{i}"]
    ends = np.cumsum(lens)
    counts = [flat[e - l: e].tolist() for e, l in zip(ends, lens)]
    assert len(counts) == n
    return GOLD[f"logits_{i}"], GOLD[f"stability_{i}"], GOLD[f"boxes_{i}"], counts


def _bits_of_rle(counts, H, W):
    """the reference's `rle_to_mask`, restated: runs in column-major order, the first one of zeros"""
    flat = np.zeros(H * W, dtype=bool)
    at, val = 0, False
    for c in counts:
        flat[at: at + c] = val
        at += c
        val = not val
    assert at == H * W
    return flat.reshape(W, H).T


def _pack_slow(bits):
    """bit k of word w of row y = bits[y, 32 w + k], LSB first, bits past W zero -- one bit at a time"""
    n, H, W = bits.shape
    out = np.zeros((n, H, packed_width(W)), dtype=np.uint32)
    for m in range(n):
        for y in range(H):
            for x in range(W):
                if bits[m, y, x]:
                    out[m, y, x // 32] |= np.uint32(1 << (x % 32))
    return out


def _same_f32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _agrees(i, rule):
    """does `rule(logits, offset) -> (records, packed)` give exactly what the reference recorded for case i?"""
    x, stab, boxes, counts = _case(i)
    n, H, W = SHAPES[i]
    rec, packed = rule(x, OFFSET)
    want_bits = np.stack([_bits_of_rle(c, H, W) for c in counts])
    ok = rec.dtype == np.int32 and rec.shape == (n, 8) and packed.dtype == np.uint32
    ok = ok and _same_f32(stability(rec), stab)
    ok = ok and rec[:, 4:].astype(np.int64).tolist() == boxes.tolist()
    ok = ok and rec[:, 0].tolist() == want_bits.sum((1, 2)).tolist()
    ok = ok and packed.shape == (n, H, packed_width(W)) and np.array_equal(packed, _pack_slow(want_bits))
    ok = ok and [r["counts"] for r in rle(packed, W)] == counts and all(r["size"] == [H, W] for r in rle(packed, W))
    ok = ok and np.array_equal(unpack(packed, W), want_bits)
    return bool(ok)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_rule_equals_the_reference(i):
    assert _agrees(i, mask_report_rule)
    x = GOLD[f"logits_{i}"]
    rec, packed = mask_report_rule(x, OFFSET)
    # the counts the reference does not return on their own, by the definition
    t = torch.from_numpy(x)
    assert rec[:, 1].tolist() == (t > OFFSET).sum((1, 2)).tolist()
    assert rec[:, 2].tolist() == (t > -OFFSET).sum((1, 2)).tolist()
    assert rec[:, 3].tolist() == (~torch.isfinite(t)).sum((1, 2)).tolist()
    # torch carries the words as int32 of the same bits
    as_i32 = torch.from_numpy(packed.view(np.int32))
    assert np.array_equal(unpack(as_i32, x.shape[2]), unpack(packed, x.shape[2]))


def test_the_inputs_hold_the_special_cases():
    seen = {"nan_stability": False, "empty": False, "nonfinite": False, "zero": False, "neg_zero": False}
    for i in range(len(SHAPES)):
        x, stab, boxes, _ = _case(i)
        rec, _ = mask_report_rule(x, OFFSET)
        seen["nan_stability"] |= bool(np.isnan(stab).any())
        seen["empty"] |= bool(((rec[:, 0] == 0) & (boxes == 0).all(1)).any())
        seen["nonfinite"] |= bool((rec[:, 3] > 0).any())
        seen["zero"] |= bool(((x == 0) & ~np.signbit(x)).any())
        seen["neg_zero"] |= bool(((x == 0) & np.signbit(x)).any())
        for v in (OFFSET, -OFFSET):
            assert i == 0 or (x == np.float32(v)).any()
    assert all(seen.values()), seen
    assert {s[2] for s in SHAPES} >= {1, 31, 33, 63, 65, 101}


def _mutant(kind):
    def rule(x, d):
        x = np.asarray(x, dtype=np.float32)
        d = np.float32(d)
        n, H, W = x.shape
        with np.errstate(invalid="ignore"):
            gt = (lambda a, b: a >= b) if kind == "ge" else (lambda a, b: a > b)
            bits = gt(x, np.float32(0))
            hi = gt(x, d)
            lo = (x >= -d) if kind == "lo_ge" else gt(x, -d)
        if kind == "nan_set":
            bits = bits | np.isnan(x)
        rec = np.zeros((n, 8), dtype=np.int32)
        rec[:, 0], rec[:, 1], rec[:, 2] = bits.sum((1, 2)), hi.sum((1, 2)), lo.sum((1, 2))
        rec[:, 3] = (~np.isfinite(x)).sum((1, 2))
        for m in range(n):
            ys, xs = np.nonzero(bits[m])
            if ys.size:
                e = 1 if kind == "exclusive_box" else 0
                rec[m, 4:] = (xs.min(), ys.min(), xs.max() + e, ys.max() + e)
        packed = pack_bits(bits)
        if kind == "msb_first":
            rev = np.zeros_like(packed)
            for k in range(32):
                rev |= ((packed >> np.uint32(k)) & np.uint32(1)) << np.uint32(31 - k)
            packed = rev
        if kind == "tail_kept" and W % 32:
            packed = packed.copy()
            packed[:, :, -1] |= np.uint32((0xFFFFFFFF << (W % 32)) & 0xFFFFFFFF)
        return rec, packed
    return rule


def test_the_restated_rule_is_the_rule():
    for i in range(len(SHAPES)):
        assert _agrees(i, _mutant("none"))


@pytest.mark.parametrize("kind", ["ge", "msb_first", "exclusive_box", "tail_kept", "lo_ge", "nan_set"])
def test_mutants_of_the_rule_fail(kind):
    failed = [SHAPES[i] for i in range(len(SHAPES)) if not _agrees(i, _mutant(kind))]
    assert failed, f"the recorded inputs cannot tell the mutant '{kind}' from the rule"


def test_refused_inputs():
    with pytest.raises(TypeError):
        mask_report_rule(np.zeros((2, 3), dtype=np.float64))
    with pytest.raises(ValueError):
        mask_report_rule(np.zeros((2, 3), dtype=np.float32), offset=-1.0)
    with pytest.raises(ValueError):
        mask_report_rule(np.zeros((2, 3), dtype=np.float32), offset=float("nan"))
    with pytest.raises(ValueError):
        unpack(np.zeros((1, 2, 2), dtype=np.uint32), 31)


# ---- the interface ------------------------------------------------------------------------------
NAMES = ("anyref_op_mask_report", "anyref_set_mask_reports", "anyref_set_packed_masks", "anyref_mask_reports")
LEDGER = {"launch_mask_report": ("op", "anyref_op_mask_report", "tests/test_gpu_mask_report_ops.py")}


def _read(rel):
    with open(os.path.join(ROOT, rel)) as f:
        return f.read()


def test_library_exports_the_symbols():
    from anyref_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the backend first (__graft_entry__.build())"
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SYMBOLS, f"{name} is not bound in anyref_amd/_lib.py"
        getattr(lib, name)          # AttributeError: not exported


def test_headers_declare_them():
    api, ops = _read("include/anyref_hip.h"), _read("include/anyref_hip_ops.h")
    assert re.search(r"^int anyref_set_mask_reports\(anyref_handle\* h, int on, float offset\);", api, re.M)
    assert re.search(r"^int anyref_set_packed_masks\(anyref_handle\* h, uint32_t\* packed_dev, int64_t cap_words\);", api, re.M)
    assert re.search(r"^int anyref_mask_reports\(anyref_handle\* h, int B, int seg_cap, int32_t\* n, int32_t\* rec, "
                     r"int64_t\* pack_offsets\);", api, re.M)
    assert re.search(r"^int anyref_op_mask_report\(void\* stream, const float\* logits, int n, int H, int W, float offset, "
                     r"int32_t\* records,\s+uint32_t\* packed\);", ops, re.M)
    assert "#define ANYREF_ABI_VERSION" in api


def test_the_launcher_has_its_ledger_line():
    declared = declared_launchers(_read("anyref_amd/csrc/mask_report.h"))
    assert declared == {"launch_mask_report"}
    problems = ledger_problems(LEDGER, declared)
    assert not problems, "\n".join(problems)
    # the launcher lives in its own header: kernels.h, whose ledger is test_cpu_glue_ops_ref's, does not declare it
    assert "launch_mask_report" not in declared_launchers(_read("anyref_amd/csrc/kernels.h"))
    # and the ledger notices a wrong line here too
    wrong = {"launch_mask_report": ("op", "anyref_op_postprocess", "tests/test_gpu_mask_report_ops.py")}
    assert any("does not call" in p for p in ledger_problems(wrong, declared))
