"""`mask_report_kernel` (csrc/mask_report.hip, through anyref_op_mask_report) against the rule in anyref_amd/maskreport.py.
Everything is integer: records and packed words must be EQUAL to the rule's, no tolerance.

Shapes (n, H, W): widths below, at and just past one and two 32-bit words and one 64-pixel unit (1, 31, 33, 63, 65, 129, 101,
64), several masks per launch, the tiny rig's 300 x 241, a mid size, and one 1024 x 1024 plane -- the only size at which a mask
takes more workgroups than the per-mask cap, so that waves stride over it.  Logits are placed 1 and 3 floats past an aligned
allocation (where masks j > 0 of an odd H * W sit in out_masks), the packed words at an odd word, and canary words on both
sides of records and packed words must survive."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anyref_amd.maskreport import mask_report_rule, packed_width, unpack  # noqa: E402

INF, NAN = float("inf"), float("nan")
SMALL = [(1, 1, 1), (1, 3, 31), (1, 5, 33), (2, 7, 63), (1, 9, 65), (1, 2, 129), (3, 37, 101), (2, 64, 64)]
SHAPES = SMALL + [(1, 300, 241), (1, 480, 640), (1, 1024, 1024)]
CANARY = -1234567
GUARD = 5


@pytest.fixture(scope="module")
def lib():
    from anyref_amd import _lib
    return _lib.load()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def planted(n, H, W, seed, d=1.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, H, W)) * 2).astype(np.float32)
    specials = [0.0, -0.0, d, -d, NAN, INF, -INF]
    for m in range(n):
        flat = x[m].reshape(-1)
        where = rng.choice(flat.size, size=min(3 * len(specials), flat.size), replace=False)
        for i, p in enumerate(where):
            flat[p] = specials[i % len(specials)]
    return x


class Bufs:
    """device buffers of one launch: logits `lead` floats past an aligned allocation, records and packed words (from an odd
    word) between canaries"""

    def __init__(self, x, lead=1, with_packed=True):
        n, H, W = x.shape
        self.n, self.H, self.W, self.Wp = n, H, W, packed_width(W)
        host = torch.full((lead + x.size + GUARD,), 3.0e4)      # what lies around the planes is > every threshold
        host[lead: lead + x.size] = torch.from_numpy(x.reshape(-1))
        self.xbuf = host.cuda()
        self.x = self.xbuf[lead:]
        self.rec = torch.full((GUARD + n * 8 + GUARD,), CANARY, dtype=torch.int32, device="cuda")
        self.pk = None
        if with_packed:
            self.pk = torch.full((GUARD + n * H * self.Wp + GUARD,), CANARY, dtype=torch.int32, device="cuda")
            assert (self.pk.data_ptr() // 4 + GUARD) % 2 == 1, "the packed words start at an odd word"

    def launch(self, lib, d=1.0, n=None, H=None, W=None, logits=True, records=True):
        return lib.anyref_op_mask_report(
            None, ptr(self.x) if logits else None, self.n if n is None else n, self.H if H is None else H,
            self.W if W is None else W, float(d), ptr(self.rec[GUARD:]) if records else None,
            None if self.pk is None else ptr(self.pk[GUARD:]))

    def read(self):
        torch.cuda.synchronize()
        rec = self.rec.cpu().numpy()
        assert (rec[:GUARD] == CANARY).all() and (rec[-GUARD:] == CANARY).all(), "a canary beside the records was written"
        out = rec[GUARD:-GUARD].reshape(self.n, 8).copy()
        if self.pk is None:
            return out, None
        pk = self.pk.cpu().numpy()
        assert (pk[:GUARD] == CANARY).all() and (pk[-GUARD:] == CANARY).all(), "a canary beside the packed words was written"
        return out, pk[GUARD:-GUARD].view(np.uint32).reshape(self.n, self.H, self.Wp).copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.rec == CANARY).all()) and (self.pk is None or bool((self.pk == CANARY).all()))


def check(lib, x, d=1.0, lead=1, with_packed=True):
    b = Bufs(x, lead, with_packed)
    rc = b.launch(lib, d)
    assert rc == 0, lib.anyref_op_last_error().decode()
    rec, pk = b.read()
    want_rec, want_pk = mask_report_rule(x, d)
    bad = np.argwhere(rec != want_rec)
    assert bad.size == 0, f"records differ at (mask, field) {bad[:4].tolist()}: got {rec[bad[0][0]]}, rule {want_rec[bad[0][0]]}"
    if with_packed:
        bad = np.argwhere(pk != want_pk)
        assert bad.size == 0, f"{len(bad)} packed words differ, the first at (mask, row, word) {bad[0].tolist()}"
    return rec, pk


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_seeded_logits_with_the_special_values(lib, shape):
    n, H, W = shape
    x = planted(n, H, W, seed=H * 1000 + W)
    for lead in ((1,) if H * W >= 1024 * 1024 else (1, 3)):
        rec, _ = check(lib, x, lead=lead)
    if H * W > 100:
        assert (rec[:, 3] > 0).all() and (rec[:, 0] > 0).all()


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 7, 63), (3, 37, 101), (1, 300, 241)], ids=str)
def test_all_negative_and_all_positive(lib, shape):
    n, H, W = shape
    neg = -np.abs(planted(n, H, W, seed=5)) - np.float32(0.25)
    neg[np.isnan(neg)] = -2.0
    rec, pk = check(lib, neg, lead=3)
    assert (rec[:, 0] == 0).all() and (rec[:, 4:] == 0).all() and not pk.any()
    rec, pk = check(lib, -neg, lead=1)
    assert (rec[:, 0] == H * W).all() and rec[:, 4:].tolist() == [[0, 0, W - 1, H - 1]] * n
    assert unpack(pk, W).all()


@pytest.mark.parametrize("shape", [(9, 65), (2, 129), (300, 241)], ids=str)
def test_single_set_pixels(lib, shape):
    H, W = shape
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + [(H // 2, c) for c in (31, 32, 63, 64, W - 1)]
    x = np.full((len(spots), H, W), -2.0, dtype=np.float32)
    for m, (r, c) in enumerate(spots):
        x[m, r, c] = 0.5
    rec, pk = check(lib, x, lead=1)
    for m, (r, c) in enumerate(spots):
        assert rec[m].tolist() == [1, 0, 1, 0, c, r, c, r]
        assert pk[m, r, c // 32] == np.uint32(1 << (c % 32)) and np.count_nonzero(pk[m]) == 1


def test_relaunch_rerun_and_no_packed_buffer(lib):
    xa, xb = planted(3, 37, 101, seed=1), planted(3, 37, 101, seed=2)
    want_b = mask_report_rule(xb, 1.0)
    b = Bufs(xa, lead=1)
    assert b.launch(lib) == 0
    first = b.read()
    assert np.array_equal(first[0], mask_report_rule(xa, 1.0)[0])
    # other logits into the same records and words, nothing cleared in between: the launcher initialises what it needs
    b.xbuf[1: 1 + xb.size] = torch.from_numpy(xb.reshape(-1)).cuda()
    assert b.launch(lib) == 0
    second = b.read()
    assert np.array_equal(second[0], want_b[0]) and np.array_equal(second[1], want_b[1])
    for _ in range(3):                                           # reruns are bit-identical
        assert b.launch(lib) == 0
        again = b.read()
        assert np.array_equal(again[0], second[0]) and np.array_equal(again[1], second[1])
    rec_only, none = check(lib, xb, lead=1, with_packed=False)   # packed = NULL: the same records
    assert none is None and np.array_equal(rec_only, second[0])


@pytest.mark.parametrize("d", [0.5, 0.0])
def test_other_offsets(lib, d):
    x = planted(2, 37, 101, seed=9, d=d if d else 1.0)
    rec, _ = check(lib, x, d=d, lead=3)
    if d == 0.0:
        assert (rec[:, 0] == rec[:, 1]).all() and (rec[:, 1] == rec[:, 2]).all()
    else:
        assert (rec[:, 1] < rec[:, 0]).all() and (rec[:, 0] < rec[:, 2]).all()


def test_refusals_leave_the_buffers_untouched(lib):
    b = Bufs(planted(1, 5, 33, seed=3), lead=1)
    refused = [dict(H=0), dict(W=0), dict(H=-1), dict(H=65536, W=32768), dict(d=-1.0), dict(d=-0.5), dict(d=NAN), dict(d=INF),
               dict(logits=False), dict(records=False)]
    for kw in refused:
        assert b.launch(lib, **kw) != 0, f"{kw} was not refused"
        assert lib.anyref_op_last_error().decode()
        assert b.untouched(), f"{kw}: refused, but something was written"
    assert b.launch(lib, n=0) == 0 and b.launch(lib, n=-2) == 0     # no masks: nothing happens
    assert b.untouched()
    assert b.launch(lib) == 0                                        # and the next launch runs
    rec, _ = b.read()
    assert np.array_equal(rec, mask_report_rule(planted(1, 5, 33, seed=3), 1.0)[0])
