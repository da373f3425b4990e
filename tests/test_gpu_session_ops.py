"""anyref_op_kv_broadcast (include/anyref_hip_ops.h): the prefix broadcast of an image session alone.  It moves bytes, so every
check is bit for bit: target rows equal row 0 on [0, P), everything else keeps the pattern it was filled with."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYERS, ROWS, MAXS = 2, 4, 37
_INT = {2: torch.int16, 4: torch.int32}


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def pattern(elem, row_elems, seed):
    """K and V caches [LAYERS, ROWS, MAXS, row_elems] filled with a running count (x 7, wrapped to the element's size; as integers:
    the kernel never interprets them), so a piece copied from or to the wrong place shows"""
    n = LAYERS * ROWS * MAXS * row_elems
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (torch.arange(n, dtype=torch.int64) * 7 + int(torch.randint(0, 1000, (1,), generator=g))).to(_INT[elem]).view(
        LAYERS, ROWS, MAXS, row_elems)
    return mk(), mk()


def call(lib, k, v, elem, row_elems, P, r0, r1, layers=LAYERS, rows=ROWS, maxs=MAXS):
    return lib.anyref_op_kv_broadcast(None, C.c_void_p(k.data_ptr()), None if v is None else C.c_void_p(v.data_ptr()), layers, rows,
                                      maxs, row_elems, elem, P, r0, r1)


# row_elems 24: rows of 48 / 96 bytes (the 16-byte path); 20 at 2 bytes: 40-byte rows, and 5: 10 / 20 bytes (the 2-byte path)
@pytest.mark.parametrize("elem", [2, 4])
@pytest.mark.parametrize("row_elems", [24, 20, 5])
@pytest.mark.parametrize("Q", [2, 3])
@pytest.mark.parametrize("P", [1, 13, MAXS])
def test_broadcast_copies_the_prefix_and_nothing_else(lib, elem, row_elems, Q, P):
    k0, v0 = pattern(elem, row_elems, seed=elem + row_elems + Q + P)
    k, v = k0.cuda(), v0.cuda()
    assert call(lib, k, v, elem, row_elems, P, 1, Q) == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()
    for got, was in ((k.cpu(), k0), (v.cpu(), v0)):
        want = was.clone()
        want[:, 1:Q, :P] = was[:, :1, :P]
        assert torch.equal(got[:, 0], was[:, 0]), "row 0 is unchanged"
        assert torch.equal(got[:, 1:Q, :P], was[:, :1, :P].expand(-1, Q - 1, -1, -1)), "target rows hold row 0's prefix"
        assert torch.equal(got, want), "positions >= P of the targets and the rows beyond them keep their pattern"


def test_later_rows_only_and_one_buffer(lib):
    """r0 = 2: a second call that grows a session from 2 to 4 queries leaves row 1 alone; vc = NULL: one buffer (the hidden rows)"""
    k0, _ = pattern(4, 24, seed=5)
    k = k0.cuda()
    assert call(lib, k, None, 4, 24, 9, 2, 4) == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()
    want = k0.clone()
    want[:, 2:4, :9] = k0[:, :1, :9]
    assert torch.equal(k.cpu(), want)


def test_vector_path_at_llama_7b_row_size(lib):
    """rows of 4096 16-bit elements, P = 300 of 512, 2 layers, 3 target rows: 2.4 MB per plane, more than one grid-stride round"""
    L, R, S, H = 2, 4, 512, 4096
    g = torch.Generator().manual_seed(9)
    k0 = torch.randint(-32768, 32767, (L, R, S, H), generator=g, dtype=torch.int16)
    v0 = torch.randint(-32768, 32767, (L, R, S, H), generator=g, dtype=torch.int16)
    k, v = k0.cuda(), v0.cuda()
    assert call(lib, k, v, 2, H, 300, 1, 4, layers=L, rows=R, maxs=S) == 0, lib.anyref_op_last_error().decode()
    torch.cuda.synchronize()
    for got, was in ((k, k0), (v, v0)):
        want = was.clone()
        want[:, 1:4, :300] = was[:, :1, :300]
        assert torch.equal(got.cpu(), want)


def test_no_op_forms_launch_nothing_and_bad_shapes_are_refused(lib):
    k0, v0 = pattern(2, 24, seed=3)
    k, v = k0.cuda(), v0.cuda()
    assert call(lib, k, v, 2, 24, 0, 1, 3) == 0            # P = 0
    assert call(lib, k, v, 2, 24, 5, 1, 1) == 0            # Q = 1: no target row
    torch.cuda.synchronize()
    assert torch.equal(k.cpu(), k0) and torch.equal(v.cpu(), v0)
    for P, r0, r1, what in ((MAXS + 1, 1, 2, b"maxS"), (-1, 1, 2, b"maxS"), (5, 0, 2, b"rows"), (5, 1, ROWS + 1, b"rows")):
        assert call(lib, k, v, 2, 24, P, r0, r1) != 0
        assert what in lib.anyref_op_last_error(), (P, r0, r1, lib.anyref_op_last_error())
    assert lib.anyref_op_kv_broadcast(None, C.c_void_p(k.data_ptr()), None, LAYERS, ROWS, MAXS, 24, 3, 5, 1, 2) != 0   # elem_size 3
    torch.cuda.synchronize()
    assert torch.equal(k.cpu(), k0) and torch.equal(v.cpu(), v0), "a refused call writes nothing"
