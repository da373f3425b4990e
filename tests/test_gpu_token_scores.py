"""Token scores through the model (include/anyref_hip.h `anyref_set_token_scores` / `anyref_token_scores`): the
log-probability and top-2 logit gap of every generated token, on the tiny config.

Bookkeeping is checked exactly, not statistically: `_return_extras` hands back the hidden states, "token g was predicted by
hidden row slen + g - 1", so the rule of anyref_amd/scores.py applied to hidden[b, slen_b + g - 1] @ lm_head.T -- float64, the
lm_head values rounded as the mode holds them -- must give the reported pair.  Bound: tests/test_gpu_stages.py holds a logit to
2 * TOL[mode] * scale; a score is a difference of two logit-sized quantities, so 4 * TOL[mode] * scale, with scale =
max(1, max |logit| of the row).  (TOL copied from that file.)  The same rule on the oracle's hidden states, same bound, in parity.

Where two runs of the backend are compared (graphs off, the switch toggled, pooled against single session, the rephrase
switch) the scores are bit-identical, as the ids are.  A drafted call's scores come from the verification pass's logits, a
GEMM instead of the step's GEMV: they are held to the plain call's within the bound above; in `perf`, where a near-tie may flip
an id between the two, up to and including the first token that differs (in `parity` none may).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from anyref_amd.config import config_tiny  # noqa: E402
from anyref_amd.scores import token_scores_rule  # noqa: E402
from oracle import anyref_oracle as O  # noqa: E402
from test_gpu_draft import Rig, T_NEW  # noqa: E402

TOL = {"parity": 2e-4, "parity16": 2e-4, "perf": 1.1e-2}      # tests/test_gpu_stages.py
MODES = ["parity", "perf"]


def lm_head_of(sd, mode):
    w = sd["lm_head.weight"].float()
    return (w if mode == "parity" else w.bfloat16().float()).double()


def rule_rows(w64, hidden_rows):
    """the rule on hidden_rows [n, H] @ w64.T -> [(id, logprob, gap, scale)]"""
    lg = hidden_rows.double().cpu() @ w64.T
    return [token_scores_rule(r.float()) + (max(1.0, r.abs().max().item()),) for r in lg]


def check_entry(mode, entry, tokens, ref, what):
    """one row's reported pairs against the rule's: lengths, the bound, and the id wherever the gap tells ids apart"""
    n = len(tokens)
    assert entry["logprob"].shape == (n,) and entry["gap"].shape == (n,), f"{what}: {entry['logprob'].shape} for {n} tokens"
    assert entry["logprob"].dtype == torch.float32 and entry["gap"].dtype == torch.float32 and not entry["gap"].is_cuda
    worst = 0.0
    for g, (rid, rlp, rgap, scale) in enumerate(ref[:n]):
        bound = 4 * TOL[mode] * scale
        elp, egap = abs(entry["logprob"][g].item() - rlp), abs(entry["gap"][g].item() - rgap)
        worst = max(worst, elp / bound, egap / bound)
        assert elp <= bound and egap <= bound, f"{what}: token {g}: logprob {entry['logprob'][g].item()} vs {rlp}, gap " \
                                               f"{entry['gap'][g].item()} vs {rgap} (bound {bound:.2e})"
        assert entry["logprob"][g] <= 0 and entry["gap"][g] >= 0
        if rgap > bound:
            assert rid == tokens[g], f"{what}: token {g} is {tokens[g]}, the rule's row says {rid} (gap {rgap})"
    print(f"    {what}: {n} tokens, worst err / bound {worst:.3f}, gaps {[round(v, 4) for v in entry['gap'].tolist()]}")


def bit_equal(a, b, what):
    assert len(a) == len(b), what
    for r, (x, y) in enumerate(zip(a, b)):
        for k in ("logprob", "gap"):
            assert x[k].shape == y[k].shape and torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), \
                f"{what}: row {r} {k} {x[k].tolist()} vs {y[k].tolist()}"


def close_to(mode, a, b, new_a, new_b, what):
    """scores of run a (drafted) against run b (plain), token by token up to and including the first id that differs"""
    for r in range(len(b)):
        same = next((i for i, (s, t) in enumerate(zip(new_a[r], new_b[r])) if s != t), len(new_b[r]))
        if mode == "parity":
            assert new_a[r] == new_b[r], f"{what}: row {r} ids {new_a[r]} vs {new_b[r]}"
        assert len(a[r]["gap"]) == len(new_a[r]), f"{what}: row {r} reports {len(a[r]['gap'])} pairs for {len(new_a[r])} tokens"
        bound = 4 * TOL[mode]                     # scale >= 1: the tightest form of the bound
        for g in range(min(same + 1, len(new_b[r]))):
            for k in ("logprob", "gap"):
                err = abs(a[r][k][g].item() - b[r][k][g].item())
                assert err <= bound, f"{what}: row {r} token {g} {k} {a[r][k][g].item()} vs {b[r][k][g].item()}"


def gen(r, **kw):
    d = r.gen(**kw)
    d["scores"] = r.m.last_token_scores()
    return d


@functools.lru_cache(maxsize=None)
def rig(mode, B):
    """one handle with the switch on, its plain answer and the rule's pairs on its hidden rows (shared, left unchanged)"""
    r = Rig(mode, B)
    r.m.set_token_scores(True)
    r.plain = gen(r)
    w = lm_head_of(r.sd, mode)
    r.ref = [rule_rows(w, r.plain["hidden"][b, r.slen[b] - 1: r.slen[b] - 1 + T_NEW]) for b in range(B)]
    print(f"[{mode} B={B}] plain answer: {r.plain['new']}")
    return r


# ----------------------------------------------------------------------------------------------------------------------
# off is off; the switch is part of the decode graph's key
# ----------------------------------------------------------------------------------------------------------------------
def same_answer(a, b, what, rows):
    """two answers bit for bit: ids, low-res logits, masks, and the hidden rows that exist (the rest of the buffer is never
    written and differs between handles)"""
    assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["low"], b["low"]), what
    assert torch.equal(a["hidden"][0, :rows], b["hidden"][0, :rows]), f"{what}: hidden rows"
    assert (a["masks"] is None) == (b["masks"] is None)
    for x, y in zip(a["masks"] or [], b["masks"] or []):
        assert torch.equal(x, y), what


@pytest.mark.parametrize("mode", MODES)
def test_off_is_off_and_toggling_never_replays_the_other_graph(mode):
    r0 = rig(mode, 1)                                           # (for its weights and its rigged config)
    never, on, both = (Rig(mode, 1, cfg=r0.cfg, sd=r0.sd) for _ in range(3))
    base = never.m.device_bytes
    assert on.m.device_bytes == base == both.m.device_bytes
    both.m.set_token_scores(False)                              # switching off what was never on allocates nothing
    assert both.m.device_bytes == base
    on.m.set_token_scores(True)
    S, MB = r0.cfg.llm.max_seq, 1
    rows = r0.slen[0] + T_NEW - 1
    assert on.m.device_bytes - base == 2 * 4 * MB * S + 4 * MB, "two f32 [max_batch, llm_max_seq] arrays and the i32 dst map"
    with pytest.raises(RuntimeError, match="token scores are off"):
        never.m.last_token_scores()
    a_off = never.gen()
    with pytest.raises(RuntimeError, match="token scores are off"):
        never.m.last_token_scores()
    a_on = gen(on)
    same_answer(a_on, a_off, "ids, hidden states and masks with the switch on and off", rows)
    assert never.m.device_bytes == base, "a call with the switch off allocates nothing for it"
    check_entry(mode, a_on["scores"][0], a_on["new"][0], r0.ref[0], f"{mode} fresh handle")
    # off, on, off, on on one handle: every call is the fresh handle's of its setting
    for i in range(4):
        both.m.set_token_scores(bool(i & 1))
        if i & 1:
            d = gen(both)
            bit_equal(d["scores"], a_on["scores"], f"call {i} (on)")
        else:
            d = both.gen()
            with pytest.raises(RuntimeError, match="token scores are off"):
                both.m.last_token_scores()
        same_answer(d, a_off, f"call {i} of off / on / off / on", rows)
    assert both.m.device_bytes == on.m.device_bytes, "switching off keeps the arrays, switching on again allocates no more"


# ----------------------------------------------------------------------------------------------------------------------
# bookkeeping against the hidden states, and against the oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 2])
def test_pairs_are_the_rule_on_the_rows_that_predicted_the_tokens(mode, B):
    r = rig(mode, B)
    assert len(set(r.slen)) == B, "rows of different prompt lengths"
    sc = r.plain["scores"]
    assert len(sc) == B
    for b in range(B):
        assert len(r.plain["new"][b]) == T_NEW
        check_entry(mode, sc[b], r.plain["new"][b], r.ref[b], f"{mode} B={B} row {b}")
    bit_equal(gen(r)["scores"], sc, "a second call")
    if mode != "parity":
        return
    with torch.no_grad():
        ref = O.anyref_generate(r.sd, r.cfg, r.clip, r.ids, r.sam, r.sizes, r.H, r.W, max_new_tokens=T_NEW, eos=False)
    w = r.sd["lm_head.weight"].double()
    for b in range(B):
        assert ref["output_ids"][b].tolist()[len(r.ids[b]):] == r.plain["new"][b]
        rows = ref["hidden"][b][r.slen[b] - 1: r.slen[b] - 1 + T_NEW]
        check_entry(mode, sc[b], r.plain["new"][b], rule_rows(w, rows), f"oracle B={B} row {b}")


@pytest.mark.parametrize("mode", MODES)
def test_eos_cuts_one_row(mode):
    r = rig(mode, 2)
    new = r.plain["new"]
    pick = [(b, g) for b in range(2) for g in range(1, T_NEW - 1) if new[b][g] not in new[b][:g] and new[b][g] not in new[1 - b]]
    assert pick, f"no id that only one row emits mid-answer: {new}"
    b, g = pick[0]
    r.m.config.eos_token_id = new[b][g]
    try:
        d = gen(r)
    finally:
        r.m.config.eos_token_id = None
    assert d["new"][b] == new[b][: g + 1] and d["new"][1 - b] == new[1 - b], (d["new"], new)
    sc = d["scores"]
    assert len(sc[b]["gap"]) == g + 1 and len(sc[1 - b]["gap"]) == T_NEW
    want = [dict(logprob=e["logprob"][: len(s["gap"])], gap=e["gap"][: len(s["gap"])]) for e, s in zip(r.plain["scores"], sc)]
    bit_equal(sc, want, "the tokens up to and including the EOS, and the other row in full")


# ----------------------------------------------------------------------------------------------------------------------
# drafts
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_drafts(mode):
    r1, r2 = rig(mode, 1), rig(mode, 2)
    V = r1.cfg.llm.vocab
    true1 = r1.plain["new"][0][:5]
    wrong = lambda d, at: d[:at] + [(d[at] + 1) % V] + d[at + 1:]
    for name, draft, accepted in (("fully accepted", true1, 5), ("corrupted at 1", wrong(true1, 1), 1),
                                  ("first token wrong", wrong(true1, 0), 0)):
        d = gen(r1, draft=[draft])
        if mode == "parity":
            assert d["accepted"] == [accepted] and d["passes"] == (0 if name == "first token wrong" else 1), (name, d["accepted"])
        assert len(d["new"][0]) == T_NEW
        close_to(mode, d["scores"], r1.plain["scores"], d["new"], r1.plain["new"], f"{mode} {name}")
        if d["new"] == r1.plain["new"]:
            check_entry(mode, d["scores"][0], d["new"][0], rule_rows(lm_head_of(r1.sd, mode),
                        d["hidden"][0, r1.slen[0] - 1: r1.slen[0] - 1 + T_NEW]), f"{mode} {name}, own hidden rows")
    true2 = [t[:5] for t in r2.plain["new"]]
    d = gen(r2, draft=[wrong(true2[0], 2), true2[1]])
    if mode == "parity":
        assert d["accepted"] == [2, 5], d["accepted"]
    close_to(mode, d["scores"], r2.plain["scores"], d["new"], r2.plain["new"], f"{mode} B=2, rows accept 2 and 5")
    # the row that got ahead went on stepping while the other finished: its pairs are still the ones of its own tokens
    if d["new"] == r2.plain["new"]:
        w = lm_head_of(r2.sd, mode)
        for b in range(2):
            check_entry(mode, d["scores"][b], d["new"][b], rule_rows(w, d["hidden"][b, r2.slen[b] - 1: r2.slen[b] - 1 + T_NEW]),
                        f"{mode} B=2 drafted row {b}, own hidden rows")


# ----------------------------------------------------------------------------------------------------------------------
# graphs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 2])
def test_eager_steps_give_the_same_bits(mode, B):
    r = rig(mode, B)
    r.m.set_graphs(False)
    try:
        d = gen(r)
        e = gen(r, draft=[t[:2] for t in r.plain["new"]])         # two accepted, three eager steps behind the pass
    finally:
        r.m.set_graphs(True)
    bit_equal(d["scores"], r.plain["scores"], f"{mode} B={B}: set_graphs(False)")
    g = gen(r, draft=[t[:2] for t in r.plain["new"]])
    bit_equal(e["scores"], g["scores"], f"{mode} B={B}: drafted, eager against graph steps")


# ----------------------------------------------------------------------------------------------------------------------
# sessions and the pool
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity", "perf", "parity16"])
def test_sessions_and_pool(mode):
    from test_gpu_session_pool import QS, prig
    r = prig(mode)
    m = r.m
    w = lm_head_of(r.sd, mode)

    def against_hidden(res, sc, ks, qs, what):
        assert len(sc) == len(ks)
        for b, (k, q) in enumerate(zip(ks, qs)):
            slen = r.P[k] + len(r.suffixes[q])
            new = r.new(res, b, k, q)
            check_entry(mode, sc[b], new, rule_rows(w, res["hidden"][b, slen - 1: slen - 1 + len(new)]), f"{what} row {b}")

    m.set_token_scores(True)
    try:
        for k in (0, 1):
            h = r.pooled([k] * 3)
            sp = m.last_token_scores()
            s = r.single(k)
            ss = m.last_token_scores()
            assert torch.equal(h["ids"], s["ids"])
            bit_equal(sp, ss, f"{mode}: pooled rows about slot {k} against a live session")
            against_hidden(h, sp, [k] * 3, QS, f"{mode} slot {k}")
        ks = (1, 0, 2)
        a = r.pooled(ks)
        against_hidden(a, m.last_token_scores(), ks, QS, f"{mode} mixed rows {ks}")
        # generate_many: two calls, rows placed by what the cache rows hold; entries come back in the caller's item order
        order = ((2, 1), (1, 0), (0, 2), (1, 3), (0, 0))
        many = r.pool.generate_many([(r.ps[k], r.suffixes[q]) for k, q in order], max_new_tokens=r.T, _return_extras=True)
        sc = m.last_token_scores()
        assert len(sc) == len(order)
        for i, (k, q) in enumerate(order):
            slen = r.P[k] + len(r.suffixes[q])
            new = many[i][0][len(r.full(k, q)):].tolist()
            assert len(new) == r.T
            check_entry(mode, sc[i], new, rule_rows(w, many[i][2]["hidden"][slen - 1: slen - 1 + len(new)]),
                        f"{mode} generate_many item {i} (image {k}, query {q})")
    finally:
        m.set_token_scores(False)
    r.pool.generate_many([(r.ps[0], r.suffixes[0])], max_new_tokens=2)
    with pytest.raises(RuntimeError, match="token scores are off"):
        m.last_token_scores()


@pytest.mark.parametrize("mode", MODES)
def test_rephrase_switch_changes_nothing_about_the_scores(mode):
    cfg = config_tiny()
    cfg.rephrase_weight = 0.1
    r = Rig(mode, 1, cfg=cfg)
    r.m.set_token_scores(True)
    off = gen(r)
    off_d = gen(r, draft=[off["new"][0][:5]])                     # (ignored off the fast paths: the plain loop)
    r.m.set_rephrase_paths(True)
    on = gen(r)
    on_d = gen(r, draft=[off["new"][0][:5]])
    assert on["new"] == off["new"] and len(off["scores"][0]["gap"]) == T_NEW
    bit_equal(on["scores"], off["scores"], f"{mode}: rephrase paths on against off")
    bit_equal(off_d["scores"], off["scores"], f"{mode}: a draft that the slow path ignores")
    close_to(mode, on_d["scores"], on["scores"], on_d["new"], on["new"], f"{mode}: drafted under the rephrase paths")
    check_entry(mode, on["scores"][0], on["new"][0], rule_rows(lm_head_of(r.sd, mode),
                on["hidden"][0, r.slen[0] - 1: r.slen[0] - 1 + T_NEW]), f"{mode} rephrase paths on")
