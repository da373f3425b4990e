"""Attention inputs with a prescribed score profile, and f32 emulations of the attention kernels in the kernels' own order
(tests/test_gpu_attn_peaked.py runs the kernels on these inputs, tests/test_cpu_attn_peaked_ref.py proves on the CPU that
the inputs reach the softmax rescale paths, that the emulation lies inside the float64 bound of
gemm_forms_ref.attention_form / test_gpu_decode_ops.decode_bound and that every mutant lies outside it).

Why: with randn operands the scores of one row stay within a few units of each other, so the running maximum of the online
softmax is fixed by the first key tile.  The 16-bit bodies of attention.hip rescale lazily -- the reference maximum moves
only when a tile's maximum exceeds it by more than 8 (log2 units), then a wave-uniform branch multiplies l and the O tiles
by exp2(m_run - mref), unmoved lanes getting 2^0 -- and none of that runs on such inputs after the first tile.

Inputs: q_i = randn + a_i hd^(1/4) u, k_j = randn + c_j hd^(1/4) u with a unit vector u of signs / sqrt(hd) and
scale = hd^-1/2 add a_i c_j (natural units) to score (i, j); cross terms ~ a_i hd^(-1/4).  v stays randn.
Row gains a_i cycle through GAINS with i % 7 (coprime with 16: every wave holds lanes that move beside lanes that do not).

Plain torch on whatever device the operands are on; nothing here needs a GPU or the HIP library.
"""
import math
from collections import namedtuple

import torch

import gemm_forms_ref as R

LOG2E = 1.4426950408889634
LAZY = 8.0                                   # the lazy rule's threshold, log2 units (attention.hip: mx > m_run + 8.f)
GAINS = (0.0, 1.0, -1.0, 0.5, 2.0, -2.0, 0.25)
PEAK = 30.0                                  # sink / spike height, natural units
TAG = {0: "attn_f32_hd", 1: "attn_bf16_hd", 2: "attn_f16_hd", 3: "attn_sp16_hd"}
SENT = -768.0                                # exact in bf16, f16 and as a pair

# ---------------------------------------------------------------------------------------------------------------------
# The cases.  dims = (B, H, Sq, Sk, hd).  bias: None, "tab" (rel-pos tables, 14 x 14 window) or "p" (P buffer, 64 x 64 grid).
# ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name tys dims causal q_pos0 q_len kv_len maxS biases profiles splits step caps")


def _case(name, tys, dims, profiles, *, causal=0, q_pos0=None, q_len=None, kv_len=None, maxS=0, biases=(None,), splits=1,
          step=0, caps=(0,)):
    return Case(name, tys, dims, causal, q_pos0, q_len, kv_len, maxS, biases, profiles, splits, step, caps)


SAM_CAPS = (0, 128, 4)       # max_wg of the 16-bit SAM forms: unset, the model's share, and one below every grid here
CASES = [
    # streaming, 4 waves x 64 keys (t = 0: 32 keys, the eager rule); keys from a cache, causal, cached prefix
    _case("stream128", (0, 1, 2, 3), (2, 2, 200, 200, 128), ("stairs", "stairs_mid", "sink"), causal=1, q_pos0=[0, 40],
          q_len=[200, 160], kv_len=[200, 200], maxS=256),
    _case("small16", (1, 2), (2, 4, 6, 196, 16), ("stairs", "spike_last"), kv_len=[196, 150]),
    # 16-bit: resident 13 waves, 5 x 48 (with the tables: 5 x 3 window rows = 42 keys); t = 3: split-pair windows, 3 x 80
    _case("window", (1, 2, 3), (1, 2, 196, 196, 80), ("stairs", "sink"), biases=(None, "tab"), caps=SAM_CAPS),
    _case("clip", (1, 2), (1, 2, 257, 257, 64), ("stairs", "stairs_mid")),
    _case("w7", (1, 2), (1, 2, 230, 230, 80), ("stairs", "spike_last")),
    # (8 query blocks over 1024 keys: the 16-bit launch splits the keys in 4, the split-pair one never does)
    _case("w8", (1, 2, 3), (1, 1, 1024, 1024, 80), ("stairs",), splits=4, caps=SAM_CAPS),
    _case("g2", (1, 2), (1, 1, 4096, 4096, 80), ("stairs", "sink"), biases=("p",), caps=SAM_CAPS),
    _case("split4", (0, 1, 2), (1, 2, 7, 1024, 16), ("stairs", "sink", "spike_last"), splits=4),
    _case("split9", (1, 2), (1, 1, 70, 2304, 32), ("stairs",), splits=9, step=256),
]
EMPTY = _case("empty", (0, 1, 2), (2, 2, 20, 70, 64), ("stairs",), kv_len=[0, 70])


def tile_width(case, ty, bias):
    """key-tile width of the form the launcher picks (attention.hip: attn_launch / attn_sp_launch)"""
    if ty == 0:
        return 32
    if case.name == "window":
        return 80 if ty == 3 else (42 if bias == "tab" else 48)      # row-padded keys: 48 slots hold 3 x 14 keys
    if case.name == "w7":
        return 80
    return 64


def want_tag(case, ty, bias):
    """(prefix, substring) of the launch tag of the form the case is meant for"""
    hd = case.dims[4]
    sub = {"window": "_w7" if ty == 3 else "_w13_res", "clip": "_res", "w7": "_w7", "w8": "_w8", "g2": "_g2w8"}.get(case.name, "")
    if ty == 3 and case.name == "stream128":
        sub = "_w4"
    return TAG[ty] + str(hd), sub


def case_splits(case, ty):
    """key splits of the launch: attn_launch_cfg's rule (case.splits); attn_sp_launch and attn_g2_launch never split"""
    return 1 if ty == 3 or case.name == "g2" else case.splits


def query_block(case):
    """queries per workgroup of the generic body: 16 x the waves of the form"""
    return 16 * {"window": 13, "w7": 7, "w8": 8}.get(case.name, 4)


def kv_splits(B, H, Sq, Sk, causal, has_kv_len, bq=64):
    """the launcher's key-split rule (attn_launch_cfg): few query blocks over many keys"""
    wgs = -(-Sq // bq) * H * B
    if causal or has_kv_len or wgs >= 128 or Sk < 1024:
        return 1
    return max(1, min(16, 256 // wgs, Sk // 256))


def key_ranges(Sk, w, splits=1):
    """[split][tile] -> (lo, hi): every split walks its chunk (a multiple of the tile width) tile by tile"""
    cdiv = lambda a, b: -(-a // b)      # noqa: E731
    chunk = cdiv(cdiv(Sk, splits), w) * w
    out = []
    for s in range(splits):
        lo, hi = s * chunk, min(Sk, (s + 1) * chunk)
        out.append([(a, min(hi, a + w)) for a in range(lo, hi, w)])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def key_profile(name, B, Sk, w, *, last=None, step=0):
    """c [B, Sk]: what a key adds to the score of a row with gain 1 (natural units).  w: the key-tile width of the form
    under test; step: the stairs' width where it is not the tile (one key split per step); last[b]: the last valid key"""
    j = torch.arange(Sk)
    c = torch.zeros(B, Sk, dtype=torch.float64)
    if name in ("stairs", "stairs_mid"):
        t = (j + (w // 2 if name == "stairs_mid" else 0)) // (step or w)
        # rows of more than 18 tiles (the 4096-token form): from the fourth period on every period starts above the last
        # one's top -- with the drift of 3 alone a period tops the one before by 4.3 log2 units, under the lazy threshold,
        # and the moves thin out to 5 % of the events
        c[:] = (7 * (t % 6) + 3 * (t // 6) + 32 * (t // 6 - 2).clamp_min(0)).double()
    elif name == "sink":
        c[:, 0] = PEAK
    elif name == "spike_last":
        for b in range(B):
            c[b, (Sk if last is None else int(last[b])) - 1] = PEAK
    else:
        raise ValueError(name)
    return c


def peaked_qkv(ty, B, H, Sq, Sk, hd, seed, c):
    """q [B, Sq, H, hd], k, v [B, Sk, H, hd] as stored (f32 values of the T-rounded operands; t = 0 / 3: f32 itself)"""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, S, H, hd, generator=g) for S in (Sq, Sk, Sk))
    u = (torch.randint(0, 2, (hd,), generator=g) * 2 - 1).float() / math.sqrt(hd)
    a = torch.tensor(GAINS)[torch.arange(Sq) % len(GAINS)]
    q = q + a[None, :, None, None] * hd ** 0.25 * u
    k = k + c.float()[:, :, None, None] * hd ** 0.25 * u
    if ty in (1, 2):
        q, k, v = (R.rnd(x, ty) for x in (q, k, v))
    return q, k, v


def case_seed(case, ty, profile, bias):
    return 1000 * sum(case.dims) + 7 * len(profile) + ord(profile[-1]) + (3 if bias else 0)


def case_inputs(case, ty, profile, bias):
    """everything of one (case, type, profile, bias) the CPU proof and the GPU test share: stored operands, tables, the tile
    width, the key ranges and the keyword arguments of attention_form / attention_kernel_order"""
    B, H, Sq, Sk, hd = case.dims
    w = tile_width(case, ty, bias)
    c = key_profile(profile, B, Sk, w, last=case.kv_len, step=case.step)
    g = torch.Generator().manual_seed(case_seed(case, ty, profile, bias) + 1)
    q, k, v = peaked_qkv(ty, B, H, Sq, Sk, hd, case_seed(case, ty, profile, bias), c)
    th = tw = None
    size = {"tab": 14, "p": 64}.get(bias, 0)
    if bias:
        th, tw = (R.rnd(torch.randn(2 * size - 1, hd, generator=g) * 0.3, ty if ty else 1) for _ in range(2))
    return dict(q=q, k=k, v=v, th=th, tw=tw, size=size, w=w, ranges=key_ranges(Sk, w, case_splits(case, ty)),
                scale=hd ** -0.5, c=c)


def rel_bias64(q, th, tw, size):
    """float64 decomposed rel-pos bias of the stored q over a size x size grid: rel_h, rel_w [B, H, S, size] and
    rel_abs = sum |q| |R| of the two dot products (what their f32 summation can lose)"""
    B, S, H, hd = q.shape
    idx = (torch.arange(size)[:, None] - torch.arange(size)[None, :] + size - 1).to(q.device)
    rq = q.double().permute(0, 2, 1, 3).reshape(B, H, size, size, hd)
    th, tw = th.double().to(q.device)[idx], tw.double().to(q.device)[idx]
    rel_h = torch.einsum("bnhwc,hkc->bnhwk", rq, th).reshape(B, H, S, size)
    rel_w = torch.einsum("bnhwc,wkc->bnhwk", rq, tw).reshape(B, H, S, size)
    rabs = [torch.einsum("bnhwc,hkc->bnhwk", rq.abs(), th.abs()).reshape(B, H, S, size),
            torch.einsum("bnhwc,wkc->bnhwk", rq.abs(), tw.abs()).reshape(B, H, S, size)]
    return rel_h, rel_w, rabs


def key_mask(B, Sq, Sk, dev, *, causal=False, kv_len=None, q_pos0=None):
    """True where key j is invisible to row i of batch b"""
    mask = torch.zeros(B, 1, Sq, Sk, dtype=torch.bool, device=dev)
    if kv_len is not None:
        for b in range(B):
            mask[b, :, :, int(kv_len[b]):] = True
    if causal:
        tri = torch.ones(Sq, Sk, dtype=torch.bool, device=dev)
        mask = mask | torch.stack([tri.triu(1 + (int(q_pos0[b]) if q_pos0 is not None else 0)) for b in range(B)])[:, None]
    return mask


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' own order, f32
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = ("o_not_rescaled", "l_not_rescaled", "wave_alpha")
SPLIT_MUTANTS = ("combine_natural_exp",)
# M taken from split 0 only: emulated too, but NOT a mutant -- any M gives the same quotient sum w O / sum w l until a weight
# leaves the f32 range, and the profiles span at most 2 x 30 natural = 87 log2 units (the CPU proof prints its ratio:
# inside the bound, as the kernel itself would be)
SPLIT_EQUIVALENT = "combine_first_max"


def _mul(ty, eq, a, b):
    """one product on the MFMA: 16-bit operands exact; t = 3: three passes over the bf16 pair terms, small terms first"""
    if ty != 3:
        return torch.einsum(eq, a, b)
    (ah, al), (bh, bl) = R.terms(a, 3), R.terms(b, 3)
    return torch.einsum(eq, al, bh) + torch.einsum(eq, ah, bl) + torch.einsum(eq, ah, bh)


def new_stats():
    return dict(events=0, moves=0, lazy_gt1=0, max_p=0.0, mixed=False, split_gap=0.0)


def attention_kernel_order(ty, q, k, v, scale, ranges, *, mask=None, bias=None, q_len=None, O0=None, o_f32=False, mutant=None,
                           stats=None):
    """f32 emulation of attn_body / attn_g2_body / attn_sp_body (attention.hip) over the stored q / k / v ([B, S, H, hd] f32):
    - t = 1 / 2 / 3: scores in log2 units, s * (scale * log2 e) (+ the bias * log2 e); the LAZY rule exactly as the kernels
      have it: m_new = mx > m_run + 8 ? mx : m_run, mref = 0 for a row that is still empty, alpha = exp2(m_run - mref)
      applied to l and O, P = exp2(s - mref) <= 2^8, rs summed from the unrounded P, P rounded to T (t = 3: split into a
      pair) before P V, the output rounded to T;
    - t = 0: natural units, the eager rule (m_new = max(m_run, mx), alpha = exp(m_run - m_new)), nothing rounded to 16 bits;
    - ranges (key_ranges): more than one split = the key-split form, every split an un-normalised partial (m, l, O) merged
      by w_s = exp2(m_s - M) (t = 0: exp), out = sum w O / sum w l (attn_combine_kernel).
    This is NOT gemm_forms_ref.attention_emulate, which keeps the textbook order (natural exp, the maximum moved by every
    tile): on peaked scores the two differ in which factors are applied when, and only this one has the kernels' branches.
    mutant: one of MUTANTS / SPLIT_MUTANTS -- o_not_rescaled, l_not_rescaled (the rescale forgets O / l), wave_alpha (the
    alpha of the first row of each 16-row group applied to the whole group), combine_natural_exp (exp where the 16-bit
    merge needs exp2); combine_first_max (M taken from split 0 only) is an equivalent form, see SPLIT_EQUIVALENT.
    stats (new_stats()): events = (row, tile >= 1 of its split) with a visible key; moves; lazy_gt1 = events without a move
    whose largest P exceeds 1; max_p; mixed = some 16-row group holds, in one tile, a row that moves and one that does not;
    split_gap = the largest difference of two splits' reference maxima of one row."""
    lazy = ty != 0
    ex = torch.exp2 if lazy else torch.exp
    B, Sq, H, hd = q.shape
    dev = q.device
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)      # noqa: E731
    s = _mul(ty, "bqhd,bkhd->bhqk", q, k) * f32(scale * LOG2E if lazy else scale)
    if bias is not None:
        s = s + bias.float() * f32(LOG2E if lazy else 1.0)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    ninf = torch.full((B, H, Sq, 1), float("-inf"), device=dev)
    zero = torch.zeros(B, H, Sq, 1, device=dev)
    G = -(-Sq // 16)

    def groups(x, fill):      # [B, H, Sq, 1] -> [B, H, G, 16]
        pad = torch.full((B, H, G * 16 - Sq, 1), fill, dtype=x.dtype, device=dev)
        return torch.cat([x, pad], 2).view(B, H, G, 16)

    parts = []
    for tiles in ranges:
        m, l, acc = ninf, zero, torch.zeros(B, H, Sq, hd, device=dev)
        for ti, (lo, hi) in enumerate(tiles):
            st = s[..., lo:hi]
            mx = st.amax(-1, keepdim=True)
            moved = (mx > m + LAZY) if lazy else (mx > m)
            m_new = torch.where(moved, mx, m)
            mref = torch.where(torch.isinf(m_new), zero, m_new)
            alpha = ex(m - mref)                                   # m = -inf -> 0; an unmoved row: 2^0 = 1
            if mutant == "wave_alpha":
                ga, gm = groups(alpha, 1.0), groups(moved, False)
                ga = torch.where(gm.any(-1, keepdim=True), ga[..., :1].expand_as(ga), torch.ones_like(ga))
                alpha = ga.reshape(B, H, G * 16, 1)[:, :, :Sq]
            p = ex(st - mref)                                      # masked: 2^-inf = 0
            rs = p.sum(-1, keepdim=True)
            pt = R.rnd(p, ty) if ty in (1, 2) else p
            l = (l if mutant == "l_not_rescaled" else l * alpha) + rs
            acc = (acc if mutant == "o_not_rescaled" else acc * alpha) + _mul(ty, "bhqk,bkhd->bhqd", pt, v[:, lo:hi])
            if stats is not None:
                stats["max_p"] = max(stats["max_p"], p.max().item())
                if ti >= 1:
                    ev = mx > float("-inf")
                    stats["events"] += int(ev.sum())
                    stats["moves"] += int((ev & moved).sum())
                    stats["lazy_gt1"] += int((ev & ~moved & (mx > mref)).sum())
                    gm, gs = groups(ev & moved, False), groups(ev & ~moved, False)
                    stats["mixed"] = stats["mixed"] or bool((gm.any(-1) & gs.any(-1)).any())
            m = m_new
        parts.append((m, l, acc))
    if len(parts) == 1:
        m, l, acc = parts[0]
        o = acc * torch.where(l > 0, 1.0 / l, zero)
    else:
        ms = torch.stack([p[0] for p in parts])
        M = ms[0] if mutant == "combine_first_max" else ms.amax(0)
        if stats is not None:
            fin = torch.isfinite(ms)
            gap = ms.masked_fill(~fin, float("-inf")).amax(0) - ms.masked_fill(~fin, float("inf")).amin(0)
            stats["split_gap"] = max(stats["split_gap"], gap[torch.isfinite(gap)].max().item())
        exw = torch.exp if mutant == "combine_natural_exp" else ex
        o, l = torch.zeros(B, H, Sq, hd, device=dev), zero
        for m, ls, acc in parts:
            wgt = torch.where(torch.isinf(m), zero, exw(m - M))
            o, l = wgt * acc + o, wgt * ls + l
        o = torch.where(l > 0, o / l, torch.zeros_like(o))
    o = R.round_out(o.permute(0, 2, 1, 3), ty, o_f32)      # (o_f32: the decode step's fallback keeps the f32 row)
    if q_len is not None:
        o = o.clone()
        for b in range(B):
            o[b, int(q_len[b]):] = O0[b, int(q_len[b]):].float()
    return o


def form_kwargs(case, x, ty, bias, dev):
    """(keyword arguments of attention_form, of attention_kernel_order) for operands already on dev"""
    B, H, Sq, Sk, hd = case.dims
    ref_kw = dict(causal=bool(case.causal), kv_len=case.kv_len, q_len=case.q_len, q_pos0=case.q_pos0, tile=x["w"])
    emu_kw = dict(mask=key_mask(B, Sq, Sk, dev, causal=bool(case.causal), kv_len=case.kv_len, q_pos0=case.q_pos0),
                  q_len=case.q_len)
    if case.q_len is not None:
        ref_kw["O0"] = emu_kw["O0"] = torch.full((B, Sq, H, hd), SENT, device=dev)
    if bias:
        rel_h, rel_w, rabs = rel_bias64(x["q"].to(dev), x["th"], x["tw"], x["size"])
        ref_kw.update(rel_h=rel_h, rel_w=rel_w, kw=x["size"], rel_abs=rabs, rel_pairs=(ty == 3 and bias == "tab"))
        emu_kw["bias"] = (rel_h[..., :, None] + rel_w[..., None, :]).reshape(B, H, Sq, Sk).float()
    return ref_kw, emu_kw


def mutant_names(case, ty, profile):
    """the mutants a case must reject (beside the dropped last key tile of the older op tests): the lazy rule's where the
    profile moves the maximum after the first tile -- a sink at key 0 fixes it in the first tile, as does a profile that is
    flat inside every key split; there the three compute
    what the kernel computes (t = 0 has no wave-uniform branch) -- and the merge's where keys are split (the natural exp
    IS the f32 merge's)"""
    moves = profile != "sink" and not case.step      # (case.step: one stair per key split, flat inside every split)
    names = [m for m in MUTANTS if ty != 0 or m != "wave_alpha"] if moves else []
    if case_splits(case, ty) > 1:
        names += [m for m in SPLIT_MUTANTS if ty != 0 or m != "combine_natural_exp"]
    return names


# ---------------------------------------------------------------------------------------------------------------------
# decode step: one query per sequence over the cache (decode_attn.h)
# ---------------------------------------------------------------------------------------------------------------------
DECODE_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
DECODE_MUTANTS = ("merge_unweighted", "batch_alpha_dropped")
DECODE_PROFILES = ("stairs", "sink", "spike_self")
DECODE_CFG = [(128, 4), (64, 4)]            # (hd, H)
DECODE_MAXS = 512
HEAD_GAINS = (1.0, 0.5, 0.0, -1.0)          # gain of head h % 4 on the profile (a head without a peak still sees a dropped key)
THETA = 10000.0


def decode_geometry(t, hd):
    """(KPI, keys per batch): LPK = hd / VEC lanes share a key, 512 / LPK keys per sweep, 6 (f32) / 4 sweeps per batch"""
    vec = 4 if t == 0 else 8
    kpi = 512 // (hd // vec)
    return kpi, kpi * (6 if t == 0 else 4)


def decode_positions(t, hd):
    kpi, batch = decode_geometry(t, hd)
    return [0, kpi, batch - 1, batch + 1, 329, DECODE_MAXS - 1]


def rope_table64(S, hd, theta=THETA):
    """[S, 2, hd / 2] f32: the table the library uploads, from the float64 formula (the CPU proof's stand-in)"""
    inv = theta ** (-torch.arange(0, hd, 2, dtype=torch.float64) / hd)
    ang = torch.arange(S, dtype=torch.float64)[:, None] * inv[None]
    return torch.stack([ang.cos(), ang.sin()], 1).float()


def decode_inputs(t, hd, H, pos, profile, tab, rotate64):
    """qkv [B, 3 H hd] f32 and the caches kc0 / vc0 / qk0 [B, maxS, H, hd] of type T.  Key j of head h is
    noise + g_j q_hat / |q_hat| with q_hat the float64 rotation of this step's q (rotate64), g_j chosen so that the added
    score follows the profile: stairs (step = the key batch), sink (key 0), spike_self (the k part of qkv is a multiple of
    the q part: the appended key, which the kernel takes from LDS, is the row's peak).  Head h takes the profile times
    HEAD_GAINS[h % 4]."""
    B, maxS = len(pos), DECODE_MAXS
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(hd * 11 + H + 5 * t + len(profile))
    qkv = torch.randn(B, 3 * H * hd, generator=g)
    kc0, vc0, qk0 = (torch.randn(B, maxS, H, hd, generator=g) * 0.5 for _ in range(3))
    x = qkv.view(B, 3, H, hd)
    n2 = (x[:, 0] ** 2).sum(-1, keepdim=True)               # the rotation keeps |q|
    hg = torch.tensor(HEAD_GAINS)[torch.arange(H) % len(HEAD_GAINS)][None, :, None]
    c = torch.zeros(maxS, dtype=torch.float64)
    if profile == "spike_self":
        x[:, 1] = x[:, 0] * hg * PEAK / (n2 * scale)
    elif profile == "sink":
        c[0] = PEAK
    else:
        c = key_profile("stairs", 1, maxS, decode_geometry(t, hd)[1])[0]
    half = hd // 2
    pd = torch.tensor(pos)
    qhat, _ = rotate64(x[:, 0, :, :half], x[:, 0, :, half:], tab[pd, 0][:, None, :], tab[pd, 1][:, None, :])
    kc0 = kc0 + (c[None, :, None, None] * (hg * qhat / (n2.double() * scale))[:, None]).float()
    return qkv, kc0.to(DECODE_DT[t]), vc0.to(DECODE_DT[t]), qk0.to(DECODE_DT[t])


def decode_append(t, qkv, pos, tab, kc0, vc0, qk0):
    """what the step stores: the f32 rotation of q / k rounded to T at row p of q_keep / kc, T(v) at row p of vc"""
    B, maxS, H, hd = kc0.shape
    half = hd // 2
    x = qkv.view(B, 3, H, hd)
    pd = torch.tensor(pos, device=qkv.device)
    bi = torch.arange(B, device=qkv.device)
    cs, sn = tab[pd, 0][:, None, :], tab[pd, 1][:, None, :]
    rot = lambda a: torch.cat([a[..., :half] * cs - a[..., half:] * sn, a[..., half:] * cs + a[..., :half] * sn], -1)  # noqa: E731
    kc, vc, qk = kc0.clone(), vc0.clone(), qk0.clone()
    qk[bi, pd], kc[bi, pd], vc[bi, pd] = (y.to(DECODE_DT[t]) for y in (rot(x[:, 0]), rot(x[:, 1]), x[:, 2]))
    return kc, vc, qk


def decode_kernel_order(t, q, kc, vc, pos, scale, *, mutant=None, stats=None):
    """f32 emulation of decode_attn_body over the stored q (q_keep row p, [B, H, hd] f32) and cache rows 0..p: key j
    belongs to lane group j % KPI; every group keeps an EAGER online-softmax state over its keys, one key batch
    (KPI x sweeps keys) at a time: mx = max(m_run, the batch's scores), alpha = exp(m_run - mx) on l and O; the KPI
    states are merged by exp(m_s - M).  mutant: merge_unweighted (the partials summed without exp(m_s - M)),
    batch_alpha_dropped (alpha = 1).  stats: group_gap = the largest difference of two lane groups' maxima of one head,
    batch_rise = the largest rise of a group's running maximum from one key batch to the next (natural units)."""
    B, H, hd = q.shape
    kpi, batch = decode_geometry(t, hd)
    dev = q.device
    outs = []
    for b, p in enumerate(pos):
        n = p + 1
        nb = -(-n // batch)
        k, v = kc[b, :n].float(), vc[b, :n].float()
        s = torch.einsum("hd,nhd->hn", q[b] * torch.tensor(scale, dtype=torch.float32, device=dev), k)
        s = torch.cat([s, torch.full((H, nb * batch - n), float("-inf"), device=dev)], 1).view(H, nb, batch // kpi, kpi)
        vv = torch.cat([v, torch.zeros(nb * batch - n, H, hd, device=dev)], 0).view(nb, batch // kpi, kpi, H, hd)
        m = torch.full((H, kpi), float("-inf"), device=dev)
        l = torch.zeros(H, kpi, device=dev)
        acc = torch.zeros(H, kpi, hd, device=dev)
        for i in range(nb):
            mx = torch.maximum(m, s[:, i].amax(1))
            seen = mx > float("-inf")
            mr = torch.where(seen, mx, torch.zeros_like(mx))
            alpha = torch.exp(m - mr)                                   # m = -inf -> 0
            if mutant == "batch_alpha_dropped":
                alpha = torch.ones_like(alpha)
            pj = torch.exp(s[:, i] - mr[:, None])                       # [H, sweeps, kpi]; masked key: 0
            l = l * alpha + pj.sum(1)
            acc = acc * alpha[..., None] + torch.einsum("huk,ukhd->hkd", pj, vv[i])
            if stats is not None and i >= 1:
                rise = (mx - m)[torch.isfinite(m)]
                if rise.numel():
                    stats["batch_rise"] = max(stats["batch_rise"], rise.max().item())
            m = mx
        M = m.amax(1, keepdim=True)
        wgt = torch.exp(m - M)                                          # empty group: exp(-inf) = 0
        if mutant == "merge_unweighted":
            wgt = torch.isfinite(m).float()
        if stats is not None:
            lo = m.masked_fill(~torch.isfinite(m), float("inf")).amin(1)
            stats["group_gap"] = max(stats["group_gap"], (m.amax(1) - lo).max().item())
        outs.append((wgt[..., None] * acc).sum(1) / (wgt * l).sum(1, keepdim=True))
    return torch.stack(outs)
