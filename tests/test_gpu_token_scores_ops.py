"""`token_scores_kernel` (csrc/ops.hip, through anyref_op_token_scores) against the rule in anyref_amd/scores.py.

Shapes: the smallest at which it can go wrong -- fewer elements than threads (N = 5), a row that is all vector body (N = 1000,
ldx = 1000), unaligned rows with a scalar head and tail (N = 4099, ldx = 4103), and the vocabulary of the checkpoints
(N = ldx = 32007: every row after the first starts off a 16-byte boundary) at one row and at nine.

What is asserted: id == torch.argmax on CPU exactly; gap bit-equal to the numpy f32 subtraction; and

    |logprob - rule| <= 2e-5 + 2^-22 * (max|x| + |logprob|)

derived for the reduction the kernel builds, not measured.  With u = 2^-24, S = sum_i exp(x_i - m), w_i = exp(x_i - m) / S the
share of entry i, d_i = m - x_i, and H = sum_i w_i d_i <= log N <= 10.4 (it is the entropy of w minus log S, S >= 1):
  * a term exp(x_i - M) is exp2((x_i - M) * log2e) on the exp unit: the subtraction and the product round the exponent by at
    most 2 d u relative to d, which is a relative error 2 d_i u of the term, plus 2u for the unit itself; weighted by the
    shares that is (2 H + 2) u <= 23 u.  (Entries with d > 30 hold less than 32007 e^-30 = 3e-9 of the sum together.)
  * a thread sums at most 8 chunks of (a + b) + (c + d) into its running sum, one rescale, and a head and a tail scalar:
    <= 14 roundings.  Every partial then passes 6 shuffle levels in its wave and 4 more in wave 0; a level is two products
    and a sum (3 roundings) and rescales the side with the smaller maximum by exp(m' - M), 2u from the unit.  Along the path of
    one entry the maxima only grow, so the exponents of its rescales add up to at most d_i: their argument errors telescope to
    another 2 d_i u, 2 H u <= 21 u weighted.  Together 14 + 10 * (3 + 2) + 21 = 85 u.
  So S is off by at most 108 u = 6.5e-6 relative, log S by as much absolutely; logf adds an ulp of a value <= 10.4 (1e-6).
  That is the 2e-5, with a factor 2.6 to spare.  lse = m + log S and logprob = x[id] - lse round once each: u * (|lse| +
  |logprob|) <= u * (max|x| + 10.4 + |logprob|), inside the 2^-22 term.  The float64 rule's own error is below 1e-12.
The chains are no longer than the ones the bound was stated for (a 32-term chain, 10 merge levels), so it stands as stated.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anyref_amd.scores import token_scores_rows  # noqa: E402

INF, NAN = float("inf"), float("nan")
SHAPES = [(1, 5, 5), (3, 1000, 1000), (5, 4099, 4103), (1, 32007, 32007), (9, 32007, 32007)]     # (M, N, ldx)
SENT_F, SENT_I = 777.0, -7
PAD = 5e4                                          # between the rows: greater than every entry, must not be read


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run(lib, x, ldx, dst=None, want_id=True, n_out=None):
    """x f32 [M, N] on the host -> (id, logprob, gap) CPU tensors, outputs pre-filled with the sentinels; also returns the row
    addresses the kernel saw (the tests place maxima relative to a row's 16-byte boundary)"""
    M, N = x.shape
    buf = torch.full((M, ldx), PAD)
    buf[:, :N] = x
    xd = buf.cuda()
    n_out = n_out or M
    lp = torch.full((n_out,), SENT_F, device="cuda")
    gap = torch.full((n_out,), SENT_F, device="cuda")
    ids = torch.full((n_out,), SENT_I, dtype=torch.int64, device="cuda") if want_id else None
    dd = None if dst is None else torch.tensor(dst, dtype=torch.int32, device="cuda")
    rc = lib.anyref_op_token_scores(None, ptr(xd), M, N, ldx, ptr(dd), ptr(lp), ptr(gap), ptr(ids))
    assert rc == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()
    return (None if ids is None else ids.cpu()), lp.cpu(), gap.cpu()


def row_split(M, N, ldx):
    """(head, tail0) per row for a buffer on a 16-byte boundary (every torch allocation is): the scalar head ends at the first
    16-byte boundary of the row, the scalar tail starts at tail0"""
    out = []
    for r in range(M):
        head = min((-(r * ldx)) % 4, N)
        out.append((head, head + (N - head) // 4 * 4))
    return out


def cases(M, N, ldx, seed):
    """name -> x [M, N]; row r of a case differs from row r - 1 in its random body"""
    g = torch.Generator().manual_seed(seed)
    base = lambda: torch.randn(M, N, generator=g) * 3.0
    out = {}
    split = row_split(M, N, ldx)
    for name, where in (("max_first", lambda r: 0), ("max_last", lambda r: N - 1),
                        ("max_after_body", lambda r: min(split[r][1], N - 1)),
                        ("max_head_end", lambda r: max(split[r][0] - 1, 0))):
        x = base()
        for r in range(M):
            x[r, where(r)] = x[r].max() + 2.0
        out[name] = x
    x = base()                                     # two equal maxima, the later one as far as it goes from the first
    for r in range(M):
        top = x[r].max() + 1.0
        x[r, (7 * r + 1) % N] = top
        x[r, N - 1 - (3 * r) % max(N // 2, 1)] = top
    out["two_maxima"] = x
    out["all_equal"] = torch.full((M, N), 1.5)
    x = torch.full((M, N), -1e4)
    for r in range(M):
        x[r, (N // 3 + 5 * r) % N] = 1e4
    out["one_hot_1e4"] = x
    x = base()
    x[torch.rand(M, N, generator=g) < 0.3] = -INF
    x[:, 0] = -INF
    x[:, N - 1] = -INF
    x[:, N // 2] = 1.0                             # (at least two finite entries... one here, one below)
    x[:, 1] = 0.5
    out["minus_inf_entries"] = x
    x = base()
    for r in range(M):
        x[r, (N // 2 + r) % N] = NAN
        x[r, N - 1] = NAN
        x[r, 1] = INF
    out["nan_row"] = x
    return out


def check_rows(x, ids, lp, gap, what):
    rid, rlp, rgap = token_scores_rows(x)
    assert torch.equal(ids, torch.argmax(x, -1)), f"{what}: ids {ids.tolist()} vs torch.argmax {torch.argmax(x, -1).tolist()}"
    assert ids.tolist() == rid.tolist(), what
    for r, (a, b) in enumerate(zip(gap.numpy(), rgap)):    # bit-equal to the f32 subtraction (NaN: any NaN)
        assert (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes(), f"{what}: row {r} gap {a!r} vs {b!r}"
    for r in range(x.shape[0]):
        a, b = float(lp[r]), float(rlp[r])
        if np.isnan(b) or np.isinf(b):
            assert (np.isnan(a) and np.isnan(b)) or a == b, f"{what}: row {r} logprob {a} vs {b}"
            continue
        finite = x[r][torch.isfinite(x[r])]
        bound = 2e-5 + 2.0 ** -22 * (float(finite.abs().max()) + abs(b))
        print(f"    {what} row {r}: logprob {a:.7f} rule {b:.7f} err {abs(a - b):.2e} (bound {bound:.2e}) gap {float(gap[r]):.6g}")
        assert abs(a - b) <= bound, f"{what}: row {r} logprob {a} vs rule {b}: err {abs(a - b):.3e} > {bound:.3e}"


@pytest.mark.parametrize("M,N,ldx", SHAPES)
def test_kernel_against_the_rule(lib, M, N, ldx):
    for name, x in cases(M, N, ldx, seed=N + M).items():
        ids, lp, gap = run(lib, x, ldx)
        check_rows(x, ids, lp, gap, f"[{M}x{N} ld {ldx}] {name}")
        if name == "one_hot_1e4":
            assert lp.tolist() == [0.0] * M and gap.tolist() == [2e4] * M, (lp, gap)
        if name == "all_equal":
            assert ids.tolist() == [0] * M and gap.tolist() == [0.0] * M
        if name == "two_maxima":
            assert gap.tolist() == [0.0] * M
        if name == "nan_row":
            assert torch.isnan(lp).all() and torch.isnan(gap).all()
        # a second run is bit-identical (no atomics, a fixed merge tree); id is optional
        ids2, lp2, gap2 = run(lib, x, ldx, want_id=False)
        assert ids2 is None
        assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32)) and torch.equal(gap.view(torch.int32), gap2.view(torch.int32))


@pytest.mark.parametrize("M,N,ldx", [(5, 4099, 4103), (9, 32007, 32007)])
def test_dst_map(lib, M, N, ldx):
    """row i writes index dst[i]; a negative entry skips the row, whose outputs keep the sentinel"""
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, N, generator=g) * 3.0
    x[1] = NAN                                     # a skipped row is not read: nothing of it can leak anywhere
    ids0, lp0, gap0 = run(lib, x, ldx)
    perm = torch.randperm(M + 2, generator=g)[:M].tolist()
    dst = [(-1 if r in (1, M - 1) else perm[r]) for r in range(M)]
    ids, lp, gap = run(lib, x, ldx, dst=dst, n_out=M + 2)
    written = {d: r for r, d in enumerate(dst) if d >= 0}
    for o in range(M + 2):
        if o in written:
            r = written[o]
            assert ids[o] == ids0[r] and lp[o].item() == lp0[r].item() and gap[o].item() == gap0[r].item(), (o, r)
        else:
            assert ids[o] == SENT_I and lp[o] == SENT_F and gap[o] == SENT_F, f"index {o} was written"
    # every row skipped: nothing is written at all
    ids, lp, gap = run(lib, x, ldx, dst=[-1] * M)
    assert (ids == SENT_I).all() and (lp == SENT_F).all() and (gap == SENT_F).all()


def test_refused_shapes_write_nothing(lib):
    x = torch.randn(2, 8).cuda()
    for M, N, ldx, word in ((2, 1, 8, "N >= 2"), (0, 8, 8, "M >= 1"), (-1, 8, 8, "M >= 1"), (2, 8, 7, "ldx < N"),
                            (2, 0, 8, "N >= 2")):
        lp = torch.full((2,), SENT_F, device="cuda")
        gap = torch.full((2,), SENT_F, device="cuda")
        ids = torch.full((2,), SENT_I, dtype=torch.int64, device="cuda")
        rc = lib.anyref_op_token_scores(None, ptr(x), M, N, ldx, None, ptr(lp), ptr(gap), ptr(ids))
        assert rc != 0 and word in lib.anyref_op_last_error().decode(), (M, N, ldx, lib.anyref_op_last_error().decode())
        torch.cuda.synchronize()
        assert (lp == SENT_F).all() and (gap == SENT_F).all() and (ids == SENT_I).all()
    lp = torch.full((2,), SENT_F, device="cuda")
    assert lib.anyref_op_token_scores(None, ptr(x), 2, 8, 8, None, ptr(lp), None, None) != 0
    assert "null" in lib.anyref_op_last_error().decode()
