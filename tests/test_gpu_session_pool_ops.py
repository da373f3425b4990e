"""anyref_op_kv_gather (include/anyref_hip_ops.h): the per-row gather / pack of a session pool alone.  It moves
bytes, so every check is bit for bit against torch indexing; both sides are filled with patterns first, so that everything outside
[0, P_b) of the rows the table names is proved untouched."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

_INT = {2: torch.int16, 4: torch.int32}


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def pattern(shape, elem, seed):
    """a running count (x 7, plus an offset, wrapped to the element's size; as integers: the kernel never interprets them), so a
    piece copied from or to the wrong place shows"""
    n = 1
    for d in shape:
        n *= d
    return (torch.arange(n, dtype=torch.int64) * 7 + seed * 1000003).to(_INT[elem]).view(*shape)


class Case:
    """working buffers k, v [layers, rows, maxS, re] (v None: one buffer) and a pool [slots, planes, maxP, re]"""

    def __init__(self, elem, row_elems, layers=2, rows=4, maxS=37, slots=3, maxP=29, two=True, seed=1):
        self.elem, self.re, self.layers, self.rows, self.maxS, self.slots, self.maxP = elem, row_elems, layers, rows, maxS, slots, maxP
        self.planes = layers * (2 if two else 1)
        self.k0 = pattern((layers, rows, maxS, row_elems), elem, seed)
        self.v0 = pattern((layers, rows, maxS, row_elems), elem, seed + 1) if two else None
        self.p0 = pattern((slots, self.planes, maxP, row_elems), elem, seed + 2)
        self.k, self.v, self.p = self.k0.cuda(), None if self.v0 is None else self.v0.cuda(), self.p0.cuda()

    def call(self, lib, table, pack=0):
        t = torch.tensor(table, dtype=torch.int32).reshape(-1, 4).contiguous()
        rc = lib.anyref_op_kv_gather(None, C.c_void_p(self.k.data_ptr()), None if self.v is None else C.c_void_p(self.v.data_ptr()),
                                     self.layers, self.rows, self.maxS, C.c_void_p(self.p.data_ptr()), self.slots, self.maxP, self.re,
                                     self.elem, C.c_void_p(t.data_ptr()), t.shape[0], pack)
        torch.cuda.synchronize()
        return rc

    def work(self, k, v):
        """both working buffers as one [planes, rows, maxS, re] tensor, K planes first (the pool's plane order)"""
        return k if v is None else torch.cat([k, v], 0)

    def check_gather(self, table):
        want = self.work(self.k0, self.v0).clone()
        for slot, P, row, skip in table:
            if not skip:
                want[:, row, :P] = self.p0[slot, :, :P]
        got = self.work(self.k.cpu(), None if self.v is None else self.v.cpu())
        assert torch.equal(got, want), "rows hold their slot's prefix on [0, P); everything else keeps its pattern"
        assert torch.equal(self.p.cpu(), self.p0), "a gather leaves the pool alone"

    def check_pack(self, table):
        w0 = self.work(self.k0, self.v0)
        want = self.p0.clone()
        for slot, P, row, skip in table:
            if not skip:
                want[slot, :, :P] = w0[:, row, :P]
        assert torch.equal(self.p.cpu(), want), "slots hold their row's prefix on [0, P); everything else keeps its pattern"
        assert torch.equal(self.work(self.k.cpu(), None if self.v is None else self.v.cpu()), w0), "a pack leaves the rows alone"


# row_elems 24: rows of 48 / 96 bytes (the 16-byte path); 20 at 2 bytes: 40-byte rows, and 5: 10 / 20 bytes (the 2-byte path)
# ragged P_b with 0 and max_prefix_rows, one slot for two rows, a skipped row; row 2 is not named at all
TABLE = [(1, 29, 0, 0), (1, 13, 3, 0), (2, 0, 1, 0)]
TABLE_SKIP = [(0, 7, 2, 0), (1, 29, 0, 1), (2, 1, 1, 0), (0, 7, 3, 0)]


@pytest.mark.parametrize("elem", [2, 4])
@pytest.mark.parametrize("row_elems", [24, 20, 5])
@pytest.mark.parametrize("table", [TABLE, TABLE_SKIP], ids=["ragged", "skip"])
def test_gather_is_torch_indexing(lib, elem, row_elems, table):
    c = Case(elem, row_elems, seed=elem + row_elems)
    assert c.call(lib, table) == 0, lib.anyref_op_last_error().decode()
    c.check_gather(table)


@pytest.mark.parametrize("elem", [2, 4])
@pytest.mark.parametrize("row_elems", [24, 5])
def test_pack_is_torch_indexing(lib, elem, row_elems):
    table = [(2, 29, 1, 0), (0, 11, 3, 0), (1, 5, 0, 1), (1, 0, 2, 0)]
    c = Case(elem, row_elems, seed=3 * elem + row_elems)
    assert c.call(lib, table, pack=1) == 0, lib.anyref_op_last_error().decode()
    c.check_pack(table)


def test_one_plane_and_many_planes(lib):
    """one buffer of one layer (the hidden rows, the image embedding: maxS = maxP = 1), and 2 x 9 planes with more rows than
    one 16-row launch takes"""
    c = Case(4, 24, layers=1, two=False, seed=11)
    t = [(0, 29, 1, 0), (2, 3, 2, 0)]
    assert c.call(lib, t) == 0, lib.anyref_op_last_error().decode()
    c.check_gather(t)
    c = Case(4, 36, layers=1, rows=3, maxS=1, slots=2, maxP=1, two=False, seed=12)
    t = [(1, 1, 0, 0), (1, 1, 2, 0)]
    assert c.call(lib, t) == 0, lib.anyref_op_last_error().decode()
    c.check_gather(t)
    c = Case(2, 8, layers=9, rows=19, maxS=21, slots=5, maxP=21, seed=13)
    t = [(r % 5, (r * 5) % 22, r, 0) for r in range(19)]
    assert c.call(lib, t) == 0, lib.anyref_op_last_error().decode()
    c.check_gather(t)


@pytest.mark.parametrize("elem", [2, 4])
def test_7b_row_size(lib, elem):
    """llm_dim 4096, two layers, a 300-row prefix: more than one workgroup per plane and row, the grid-stride loop's four-deep body
    and its tail"""
    c = Case(elem, 4096, layers=2, rows=2, maxS=320, slots=2, maxP=301, seed=17)
    t = [(1, 300, 0, 0), (0, 301, 1, 0)]
    assert c.call(lib, t) == 0, lib.anyref_op_last_error().decode()
    c.check_gather(t)


@pytest.mark.parametrize("elem,row_elems", [(2, 24), (4, 5)])
def test_pack_then_gather_round_trip(lib, elem, row_elems):
    c = Case(elem, row_elems, seed=23)
    assert c.call(lib, [(2, 17, 1, 0), (0, 29, 3, 0)], pack=1) == 0, lib.anyref_op_last_error().decode()
    assert c.call(lib, [(2, 17, 0, 0), (0, 29, 2, 0), (2, 17, 3, 0)]) == 0, lib.anyref_op_last_error().decode()
    w0, got = c.work(c.k0, c.v0), c.work(c.k.cpu(), c.v.cpu())
    want = w0.clone()
    want[:, 0, :17] = w0[:, 1, :17]
    want[:, 2, :29] = w0[:, 3, :29]
    want[:, 3, :17] = w0[:, 1, :17]
    assert torch.equal(got, want)
    # a rerun moves the same bytes
    assert c.call(lib, [(2, 17, 0, 0), (0, 29, 2, 0), (2, 17, 3, 0)]) == 0
    assert torch.equal(c.work(c.k.cpu(), c.v.cpu()), want)


def test_refused_shapes_launch_nothing(lib):
    c = Case(2, 24, seed=29)
    bad = [([(0, 30, 0, 0)], b"P outside"),          # P_b > max_prefix_rows
           ([(0, -1, 0, 0)], b"P outside"),
           ([(0, 5, 4, 0)], b"row outside"),         # row index out of range
           ([(0, 5, -1, 0)], b"row outside"),
           ([(3, 5, 0, 0)], b"slot outside"),
           ([(0, 5, 1, 0), (1, 5, 1, 0)], b"one row"),          # two slots into one row
           ([(0, 5, 0, 0), (1, 29, 9, 1)], b"row outside")]     # a skipped item is checked too
    for table, what in bad:
        assert c.call(lib, table) != 0, table
        assert what in lib.anyref_op_last_error(), (table, lib.anyref_op_last_error())
    assert c.call(lib, [(0, 5, 1, 0), (0, 5, 2, 0)], pack=1) != 0 and b"one slot" in lib.anyref_op_last_error()
    # P_b > maxS with a pool that would take it
    c2 = Case(2, 24, maxS=9, maxP=29, seed=31)
    assert c2.call(lib, [(0, 10, 0, 0)]) != 0 and b"P outside" in lib.anyref_op_last_error()
    for cc in (c, c2):
        cc.check_gather([])                          # nothing moved on either side
    # an empty table and an all-skipped one are no error and move nothing
    assert c.call(lib, []) == 0 and c.call(lib, [(0, 5, 1, 1), (1, 0, 2, 0)]) == 0
    c.check_gather([])
