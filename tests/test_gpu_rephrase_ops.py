"""Kernel-level test of the fused rephrase launch pair (include/anyref_hip_ops.h `anyref_op_seg_rephrase`)
against the float64 restatement in tests/rephrase_ref.py, computed over exactly the stored operands.

The allowance is derived there (`rel_bound`), from the f32 arithmetic of the two passes, and applied per element to
weight * sum_j |w_j hidden_jd| / tot.  Everything an item may not read -- query rows other than e0, key rows past e0, hidden rows
outside [s0, e0), the scratch -- is NaN, so a read past the key count or the span shows in the result."""
import ctypes as C

import pytest
import torch

import rephrase_ref as R

pytestmark = pytest.mark.gpu

_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
MAXS, NB, ROWS, CAP = 512, 3, 6, 64
# (s0, e0): span 2 at the start; span 1; one key past a 256-key sweep; mid-cache; the last row of the cache with span 64
SPANS = [(0, 2), (4, 5), (250, 257), (291, 300), (447, 511)]
WEIGHT = 0.5


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr())


def make_case(t, heads, hd, items, seed):
    """operands with NaN wherever the items may not read; the y row of an item holds half the term's magnitude (random sign), so
    the rounding of the final add stays inside the bound's last summand; the other rows hold noise.
    -> q, k, hidden, y0, [(term, bound) per item], scale"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    D = heads * hd
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    q = torch.full((NB, MAXS, heads, hd), float("nan"), device="cuda", dtype=_DT[t])
    k = torch.full((NB, MAXS, heads, hd), float("nan"), device="cuda", dtype=_DT[t])
    hidden = torch.full((NB, MAXS, D), float("nan"), device="cuda")
    for b, e0, s0, _ in items:
        q[b, e0] = rn(heads, hd).to(_DT[t])
        k[b, : e0 + 1] = rn(e0 + 1, heads, hd).to(_DT[t])
        hidden[b, s0:e0] = rn(e0 - s0, D)
    y0 = rn(ROWS, D)
    ref = []
    scale = hd ** -0.5
    for it in items:
        b, e0, s0, row = it
        term, bound = R.seg_rephrase(q, k, hidden, it, scale, WEIGHT)
        p, _ = R.pass_a(q[b, e0], k[b], e0, scale)
        mag = R.pass_b(p, hidden[b], s0, e0, WEIGHT)[1]
        y0[row] = (0.5 * mag * torch.where(rn(D) < 0, -1.0, 1.0)).float()
        ref.append((term, bound))
    return q, k, hidden, y0, ref, scale


def run(lib, t, heads, hd, q, k, hidden, y, items, scale, span_cap=CAP, max_span=None):
    it = torch.tensor(items, dtype=torch.int32, device="cuda")
    scratch = torch.full((len(items), heads, span_cap), float("nan"), device="cuda")
    launched = C.c_int32(-1)
    ms = max(e0 - s0 for _, e0, s0, _ in items) if max_span is None else max_span
    rc = lib.anyref_op_seg_rephrase(t, None, P(q), P(k), MAXS, heads, hd, P(hidden), P(it), len(items), ms, span_cap, P(scratch),
                                    scale, WEIGHT, P(y), C.byref(launched))
    assert rc == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()
    return launched.value


def check_launch(lib, t, heads, hd, items, seed, what):
    q, k, hidden, y0, ref, scale = make_case(t, heads, hd, items, seed)
    y = y0.clone()
    assert run(lib, t, heads, hd, q, k, hidden, y, items, scale) == 1, what
    worst = 0.0
    touched = set()
    for (b, e0, s0, row), (term, bound) in zip(items, ref):
        want = y0[row].double() + term
        assert torch.isfinite(y[row]).all(), f"{what}: item {(b, e0, s0, row)} read a NaN (past the keys or the span)"
        worst = max(worst, ((y[row].double() - want).abs() / bound).max().item())
        touched.add(row)
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, f"{what}: worst error / bound = {worst:.3f}"
    for r_ in range(ROWS):
        if r_ not in touched:
            assert torch.equal(y[r_], y0[r_]), f"{what}: y row {r_} of another slot changed"
    again = y0.clone()
    assert run(lib, t, heads, hd, q, k, hidden, again, items, scale) == 1
    assert torch.equal(again, y), f"{what}: a second run differs"
    return worst


@pytest.mark.parametrize("heads", [4, 5, 40])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("t", [0, 1, 2])
def test_seg_rephrase_against_float64(lib, t, hd, heads):
    """one item per launch for every span of SPANS, then three items in one launch (different images, lengths, output rows)"""
    seed = 1000 * t + 10 * hd + heads
    for i, (s0, e0) in enumerate(SPANS):
        check_launch(lib, t, heads, hd, [(i % NB, e0, s0, (2 * i + 1) % ROWS)], seed + i, f"t={t} hd={hd} heads={heads} span=({s0},{e0})")
    three = [(2, 257, 250, 4), (0, 511, 447, 0), (1, 5, 4, 3)]
    check_launch(lib, t, heads, hd, three, seed + 7, f"t={t} hd={hd} heads={heads} three items")


def test_the_bound_sees_a_dropped_key_and_a_shifted_span():
    """mutants of the reference: the key e0 left out of the softmax, and the span taken one row late -- each breaks the
    bound somewhere, so the bound is tight enough to see them (float64 only; no kernel involved)"""
    g = torch.Generator().manual_seed(5)
    heads, hd, s0, e0 = 4, 64, 291, 300
    q = torch.randn(1, MAXS, heads, hd, generator=g)
    k = torch.randn(1, MAXS, heads, hd, generator=g)
    hidden = torch.randn(1, MAXS, heads * hd, generator=g)
    scale = hd ** -0.5
    term, bound = R.seg_rephrase(q, k, hidden, (0, e0, s0, 0), scale, WEIGHT)
    p, _ = R.pass_a(q[0, e0], k[0], e0 - 1, scale)                             # keys [0, e0 - 1]
    dropped, _ = R.pass_b(torch.cat([p, p[:, :1] * 0], 1), hidden[0], s0, e0, WEIGHT)
    p_full, _ = R.pass_a(q[0, e0], k[0], e0, scale)
    shifted, _ = R.pass_b(p_full, hidden[0], s0 + 1, e0, WEIGHT)
    assert ((shifted - term).abs() / bound).max() > 1
    # dropping a key rescales every p_h by its own factor: visible unless all heads' factors agree
    assert ((dropped - term).abs() / bound).max() > 1


@pytest.mark.parametrize("t,hd,why", [(2, 20, "40-byte rows"), (0, 24, "six 16-byte pieces"), (1, 64, "span past the scratch")])
def test_refused_shapes_write_nothing(lib, t, hd, why):
    heads = 4
    D = heads * hd
    q = torch.randn(NB, MAXS, heads, hd, device="cuda").to(_DT[t])
    k = torch.randn(NB, MAXS, heads, hd, device="cuda").to(_DT[t])
    hidden = torch.randn(NB, MAXS, D, device="cuda")
    y0 = torch.randn(ROWS, D, device="cuda")
    y = y0.clone()
    items = [(0, 300, 291, 1)]
    got = run(lib, t, heads, hd, q, k, hidden, y, items, hd ** -0.5, span_cap=8 if "scratch" in why else CAP)
    assert got == 0, why
    assert torch.equal(y, y0), f"{why}: a refused launch wrote y"
