"""anyref_op_draft_accept (include/anyref_hip_ops.h): the accept step of the draft-verified greedy decode against a torch
restatement of its rule, on planted logits.  Everything it leaves is an integer or a copied table row, so every check is
exact."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

B, K, D_EMB, MAXS = 3, 5, 96, 640
_TABLE_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def plant(N, layout, g):
    """logits [B, K, N] in [-1, 1) with planted maxima, first tokens and drafts; -> (logits, t0 [B], draft [B, K], lens [B], what)"""
    x = torch.rand(B, K, N, generator=g) * 2 - 1
    want = torch.randint(0, N, (B, K), generator=g)          # the model's choice behind each fed token
    want[:, 3] = N - 1                                       # the last column once (the scalar tail when N % 4 != 0)
    want[:, 1] = 0
    for b in range(B):
        for i in range(K):
            x[b, i, want[b, i]] = 2.0
    t0 = torch.randint(0, N, (B,), generator=g)
    true = torch.cat([t0[:, None], want[:, : K - 1]], 1)     # the draft that is accepted in full: g[0 .. K)
    draft, lens = true.clone(), torch.full((B,), K, dtype=torch.int32)
    if layout == "A":
        # row 0: full acceptance through an exact tie (the same value at a lower and a higher index: the lower one is chosen and
        # is what the draft holds); row 1: t0 mismatch; row 2: zero-length
        lo, hi = 17, N - 5
        x[0, 2, :] = x[0, 2, :].clamp(max=1.0)
        x[0, 2, lo] = x[0, 2, hi] = 3.0
        want[0, 2] = lo
        draft[0, 3] = lo
        draft[1, 0] = (t0[1] + 1) % N
        lens[2] = 0
        what = dict(accepted=[K, 0, 0])
    else:
        # row 0: mismatch at index 2; row 1: a tie whose HIGHER index is in the draft (index 1 of the draft: rejected there,
        # the lower index is the model's token); row 2: full acceptance of a shorter draft (3 of K)
        draft[0, 2] = (true[0, 2] + 1) % N
        lo, hi = 4, 5
        x[1, 0, :] = x[1, 0, :].clamp(max=1.0)
        x[1, 0, lo] = x[1, 0, hi] = 3.0
        want[1, 0] = lo
        draft[1, 1] = hi
        lens[2] = 3
        what = dict(accepted=[2, 1, 3])
    return x, t0, draft, lens, what


def restate(x, t0, draft, lens):
    """the rule in torch: p = argmax per row (first index on ties); g[0] = t0, g[j + 1] = p[j]; m = leading matches"""
    p = torch.argmax(x, -1)
    acc, toks = [], []
    for b in range(B):
        gtok, m = [int(t0[b])], 0
        while m < int(lens[b]) and gtok[m] == int(draft[b, m]):
            gtok.append(int(p[b, m]))
            m += 1
        acc.append(m)
        toks.append(gtok)
    return p, acc, toks


# vocab 1000 on the 16-byte path, 1003 at an unaligned row stride (the scalar path), each with the three table types and both
# layouts; vocab 32000 -- one full float4 sweep of the 1024-thread row scan -- once
CASES = [(N, ldx, dt, lay) for N, ldx in ((1000, 1000), (1003, 1005)) for dt in (0, 1, 2) for lay in "AB"] + [(32000, 32000, 1, "A")]


@pytest.mark.parametrize("N,ldx,dtype,layout", CASES)
def test_draft_accept(lib, N, ldx, dtype, layout):
    g =torch.Generator().manual_seed(N + 7 * dtype + (layout == "B"))
    x, t0, draft, lens, what = plant(N, layout, g)
    p_ref, acc_ref, tok_ref = restate(x, t0, draft, lens)
    assert acc_ref == what["accepted"], (acc_ref, what)       # the planted scenario is the one the restatement sees
    buf = torch.full((B * K, ldx), 9.0)                      # beyond N: larger than every entry, must not be read
    buf[:, :N] = x.reshape(B * K, N)
    table = torch.randn(N, D_EMB, generator=g).to(_TABLE_DT[dtype])
    pos0 = torch.tensor([300, 17, MAXS - K - 2], dtype=torch.int32)
    dev = lambda t: t.cuda()
    logits, tab_d, draft_d, lens_d = dev(buf), dev(table), dev(draft), dev(lens)
    nxt, pos = dev(t0.clone()), dev(pos0.clone())
    p = torch.full((B * K,), -7, dtype=torch.int64, device="cuda")
    tokens = torch.full((B, K + 1), -7, dtype=torch.int64, device="cuda")
    accepted = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    x_next = torch.full((B, D_EMB), float("nan"), device="cuda")
    row_map = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    kvlen = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.anyref_op_draft_accept(None, ptr(logits), B, K, N, ldx, ptr(p), ptr(draft_d), ptr(lens_d), ptr(nxt), ptr(pos),
                                    ptr(tokens), ptr(accepted), ptr(tab_d), dtype, D_EMB, MAXS, ptr(x_next), ptr(row_map),
                                    ptr(kvlen))
    assert rc == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(p.cpu().view(B, K), p_ref), "row argmaxes (first index on ties)"
    assert accepted.cpu().tolist() == acc_ref
    tok = tokens.cpu()
    for b in range(B):
        m = acc_ref[b]
        assert tok[b, : m + 1].tolist() == tok_ref[b], f"row {b}: tokens g[0 .. m]"
        assert tok[b, m + 1:].tolist() == [-7] * (K - m), f"row {b}: nothing past g[m] is written"
        assert int(nxt[b]) == tok_ref[b][m], f"row {b}: next = g[m]"
        assert int(pos[b]) == int(pos0[b]) + m, f"row {b}: pos += m"
        assert int(row_map[b]) == b * MAXS + int(pos0[b]) + m and int(kvlen[b]) == int(pos0[b]) + m + 1, f"row {b}"
        assert torch.equal(x_next[b].cpu(), table[tok_ref[b][m]].float()), f"row {b}: x_next is the table row of g[m], bit for bit"


def test_draft_accept_refuses_k_outside_its_range(lib):
    z = torch.zeros(8, dtype=torch.int64, device="cuda")
    f = torch.zeros(64, device="cuda")
    i = torch.zeros(8, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for k in (0, 257):
        rc = lib.anyref_op_draft_accept(None, ptr(f), 1, k, 8, 8, ptr(z), ptr(z), ptr(i), ptr(z), ptr(i), ptr(z), ptr(i), ptr(f), 0,
                                        8, 16, ptr(f), ptr(i), ptr(i))
        assert rc != 0 and b"k" in lib.anyref_op_last_error()
