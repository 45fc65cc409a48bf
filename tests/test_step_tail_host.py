"""CPU: the references, inputs and item lists of tests/test_step_tail_gpu.py (step_tail_fixture).

The exact reduction reference is held against Python-integer sums and against math.fsum over the
source read through the header's own contract; the layout has NaN outside every footprint and the
sentinel outside every output; the "wide" family is one an fp32 accumulation does not reproduce and
the "once" family one it does; the hand-made lists reach the branch of segment_sum they are named
after; the engine's own reduction items (traced on the CPU) contain all four branches.  The AdamW
reference's inputs meet their conditions, the bounds are tight enough to see the step, and a
float32 restatement of the kernel stays inside them.  Needs the built library (the trace's host
queries), no GPU.
"""
import collections
import math

import numpy as np
import pytest

import step_tail_fixture as sf


def _small(items, limit=20000, n=6):
    return [it for it in items if it.count * it.len <= limit][:n]


SELF_CHECK = (_small(sf.vec_items(12)) + _small(sf.vec_items(64)) + _small(sf.scalar_items(5))
              + _small(sf.scalar_items(27)[20:]) + _small(sf.f64_items()) + _small(sf.f64_items()[30:])
              + _small(sf.near_miss_items(), n=8))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("family", sf.FAMILIES)
def test_reference_equals_integer_and_fsum_sums(family, acc):
    prob = sf.build(SELF_CHECK, family, acc=acc, keep=True)
    src64 = prob.src.view(np.float64)
    bits = lambda a: np.asarray(a, dtype=np.float32).view(np.int32)   # noqa: E731
    for row, (q, prior, scale) in zip(prob.rows.tolist(), prob.qs):
        so, cnt, ist, tst, ln, do, a, f64 = row
        assert a == acc and q.shape == (cnt, ln)
        s = src64 if f64 else prob.src
        for t in range(ln):
            # Python integers, rounded once: int -> float is exact below 2^53, the scale a power of 2
            total = sum(int(x) for x in q[:, t]) + (int(prior[t]) if acc else 0)
            assert abs(total) < 2 ** 53
            want = np.float32(float(total) * scale)
            # the header's contract on the source itself, exactly rounded by fsum
            terms = [float(s[so + i * ist + t * tst]) for i in range(cnt)]
            if acc:
                terms.append(float(prob.dst0[do + t]))
            assert not any(math.isnan(x) for x in terms)
            got = np.float32(math.fsum(terms))
            e = prob.expect[do + t]
            assert bits(want) == bits(e) == bits(got), (row, t, want, e, got)


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_nan_outside_footprints_and_sentinel_outside_outputs(family):
    items = SELF_CHECK + sf.scalar_items(3)[:12]
    prob = sf.build(items, family, acc=1)
    own = np.zeros(prob.src.size, dtype=bool)       # fp32 words some item reads
    dspan = np.zeros(prob.src.size // 2, dtype=bool)  # doubles inside an fp64 item's span
    for so, cnt, ist, tst, ln, do, a, f64 in prob.rows.tolist():
        idx = (so + np.arange(cnt)[:, None] * ist + np.arange(ln)[None, :] * tst).ravel()
        assert np.unique(idx).size == idx.size       # a footprint does not fold onto itself
        w = np.concatenate((2 * idx, 2 * idx + 1)) if f64 else idx
        assert not own[w].any()                      # nor onto another item's
        own[w] = True
        vals = (prob.src.view(np.float64) if f64 else prob.src)[idx]
        assert np.all(np.isfinite(vals)) and np.all(vals != 0)
        if f64:
            dspan[so:so + (cnt - 1) * ist + (ln - 1) * tst + 1] = True
    # every other word is NaN as a float, and inside an fp64 span as a double too
    assert np.all(np.isnan(prob.src[~own & ~np.repeat(dspan, 2)]))
    gaps64 = dspan & ~own[0::2]
    assert gaps64.any() and np.all(np.isnan(prob.src.view(np.float64)[gaps64]))
    assert prob.src.size % 4 == 0 and prob.src.size <= sf.MAX_WORDS
    cov = prob.covered()
    assert cov.sum() == sum(ln for _, ln in prob.outs)          # disjoint outputs
    assert not cov[0] and not cov[-1]
    assert np.all(prob.dst0.view(np.int32)[~cov] == sf.SENTINEL)
    assert np.all(prob.expect.view(np.int32)[~cov] == sf.SENTINEL)
    # the prior dst of an accumulating item is an exact value of the family, never the sentinel
    assert np.all(np.isfinite(prob.dst0[cov])) and np.all(np.isfinite(prob.expect[cov]))
    compact = sf.build(items, family, acc=0, gaps=False)
    assert compact.covered().all() and np.all(compact.dst0.view(np.int32) == sf.SENTINEL)


def _fp32_accumulation(prob, k):
    """Item k of prob summed term after term in fp32 (np.cumsum adds sequentially)."""
    so, cnt, ist, tst, ln, do, a, f64 = prob.rows[k].tolist()
    s = prob.src.view(np.float64) if f64 else prob.src
    x = s[so + np.arange(cnt)[:, None] * ist + np.arange(ln)[None, :] * tst].astype(np.float32)
    return np.cumsum(x, axis=0, dtype=np.float32)[-1], prob.expect[do:do + ln]


def test_an_fp32_accumulation_shows_in_the_wide_family_only():
    """A condition on the inputs, not a measurement of the kernel: the wide family must be one an
    fp32 accumulation gets wrong on more than half of the outputs (fp32 and fp64 sources), the once
    family one it gets right on all of them."""
    items = [sf.item(864, 64, 1, 64), sf.item(1728, 44, 1, 32), sf.item(108, 17, 1, 16, f64=1),
             sf.item(4096, 3, 4096 * 3, 8, f64=1), sf.item(12289, 3, 1, 1, mod=1)]
    wide, once = sf.build(items, "wide"), sf.build(items, "once")
    for k, it in enumerate(items):
        got, want = _fp32_accumulation(wide, k)
        share = float(np.mean(got.view(np.int32) != want.view(np.int32)))
        assert share > 0.5, (it, share)
        got, want = _fp32_accumulation(once, k)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), it
    got, want = _fp32_accumulation(wide, 0)
    print(f"fp32 accumulation of 864 x 64 wide terms: {int(np.sum(got != want))} of 64 outputs differ")


def test_order_family_tells_the_forms_apart():
    """The order-dependent sums: each item's expected bits are its own form's order of additions,
    and on every near-miss group with more than a handful of terms the float4 order and the scalar
    order differ on more than half of the outputs (so an item that takes the wrong form is seen).
    order_sum itself is held against a term-by-term Python restatement of segment_sum's threads."""
    prob = sf.build(sf.near_miss_items(), "order", keep=True)
    f32bits = lambda a: np.asarray(a, dtype=np.float32).view(np.int32)   # noqa: E731
    k = 0
    for base, var in sf.near_miss_groups():
        x = prob.qs[k][0]
        t4, ts = 256 // (base.len // 4), 256 // base.len
        assert (sf.tp(base), sf.tp(var[0]), sf.tp(var[1])) == (t4, ts, ts)
        e4, es = sf.order_sum(x, t4), sf.order_sum(x, ts)
        do, ln = prob.outs[k]
        assert np.array_equal(f32bits(prob.expect[do:do + ln]), f32bits(e4))
        for j in (1, 2):
            dv, lv = prob.outs[k + j]
            assert np.array_equal(prob.qs[k + j][0], x)
            assert np.array_equal(f32bits(prob.expect[dv:dv + lv]), f32bits(es))
        if base.count >= 33:
            assert np.mean(f32bits(e4) != f32bits(es)) > 0.5, base
            # and neither is the exact sum: the inputs do depend on the order
            exact = np.array([math.fsum(x[:, t]) for t in range(ln)])
            assert np.mean(f32bits(exact) != f32bits(es)) > 0.5
        k += 1 + len(var)
    # order_sum against the kernel's loops, thread by thread
    x = sf.draw_order(np.random.default_rng(5), (75, 6))
    for t in (1, 4, 42, 256):
        red = [[0.0] * 6 for _ in range(t)]
        for kk in range(t):
            for i in range(kk, 75, t):
                for o in range(6):
                    red[kk][o] = red[kk][o] + float(x[i, o])
        want = [0.0] * 6
        for kk in range(t):
            for o in range(6):
                want[o] = want[o] + red[kk][o]
        assert np.array_equal(sf.order_sum(x, t), np.array(want))


def test_hand_lists_reach_their_forms_and_fit_the_source_cap():
    lists = sf.hand_lists()
    for ln in sf.VEC_LENS:
        its = lists[f"vec{ln}"]
        t = 256 // (ln // 4)
        assert {sf.branch(it) for it in its} == {"float4"} and {sf.tp(it) for it in its} == {t}
        assert {it.count for it in its} >= {1, t, t + 1, 8 * t, 8 * t + 1, 864, 1728}
        assert {it.istride == ln for it in its} == {True, False}
    for ln in sf.SCALAR_LENS:
        its = lists[f"scalar{ln}"]
        t = 256 // ln
        assert {sf.branch(it) for it in its} == {"scalar", "scalar_long"}
        assert {it.count for it in its} >= {sf.SEG_LONG * t, sf.SEG_LONG * t + 1, 8 * t, 16 * t + 1}
        assert {it.tstride for it in its} >= {1, 3} and any(it.tstride == 3 * it.count for it in its)
    assert {sf.branch(it) for it in lists["f64"]} == {"fp64"}
    assert {it.count for it in lists["f64"]} == {1, 7, 8, 9, 108, 864, 4096}
    for base, var in sf.near_miss_groups():
        assert sf.branch(base) == "float4" and "float4" not in {sf.branch(v) for v in var}
        assert [v.mod % 4 for v in var] == [1, 0, 0] and var[1].istride % 4 == 2
        assert var[2].len == base.len - 1
    for name, its in lists.items():
        for chunk in sf.chunks(its):
            assert sf.build(chunk, "once").src.size <= sf.MAX_WORDS + 4096, name
    mixed = sf.mixed_items()
    assert len(mixed) == 3000 and mixed[:100] == sf.mixed_items(100)
    assert {sf.branch(it) for it in mixed} == {"float4", "scalar", "scalar_long", "fp64"}
    assert sf.build(mixed, "wide", gaps=False).src.size <= sf.MAX_WORDS


def test_engine_items_contain_every_branch():
    """An engine change that stops emitting one of segment_sum's four forms is seen here."""
    its = sf.engine_items()
    assert len({sf.signature(it) for it in its}) == len(its) >= 100
    forms = collections.Counter(sf.branch(it) for it in its)
    print(f"engine signatures: {len(its)}, by branch {dict(forms)}")
    assert set(forms) == {"float4", "scalar", "scalar_long", "fp64"}
    # the lists the issue names: the 864- / 1728-long float4 rows, the long one-channel depthwise list
    assert any(sf.branch(it) == "float4" and it.count == 1728 for it in its)
    assert any(sf.branch(it) == "scalar_long" and it.len == 27 for it in its)
    assert all(it.len <= 256 and it.count >= 1 for it in its)
    # every signature can be re-based: its footprint does not fold onto itself
    for it in its:
        if it.tstride == 1:
            assert it.istride >= it.len or it.count == 1, it
        else:
            assert it.tstride >= it.count * it.istride or it.istride >= it.len * it.tstride, it


# ------------------------------------------------------------------ AdamW
def test_adamw_inputs_meet_their_conditions():
    n = 217229
    p, g, m, v = sf.adamw_inputs(n)
    assert np.all(p[:n // 2] == 0) and np.all(p[(n + 1) // 2:] != 0)
    nz = np.abs(g[g != 0])
    assert nz.min() >= 2.0 ** -40 and 5.5 <= np.log10(nz.max() / nz.min()) <= 6.0
    i = np.arange(n)
    assert np.all((g == 0) == (i % 11 == 10))
    assert np.all((m == 0) == (i % 7 == 6)) and np.all((v == 0) == (i % 7 == 6)) and np.all(v >= 0)
    p1, g1, m1, v1 = sf.adamw_inputs(n, zero_moments=True)
    assert not m1.any() and not v1.any() and np.array_equal(g1, g)
    assert sf.adamw_inputs(1)[0][0] == 0 and sf.adamw_inputs(1)[1][0] != 0


@pytest.mark.parametrize("t", sf.ADAMW_STEPS)
def test_adamw_bounds_see_the_step_and_leave_fp32_room(t):
    """On at least 95 % of the elements with a non-zero reference step the bound on a zero-valued
    parameter is below 1e-3 of that step (the test stays sensitive), and a float32 restatement of
    the kernel is inside every bound (the device's powf has room)."""
    n = 217229
    p, g, m, v = sf.adamw_inputs(n, zero_moments=(t == 1))
    worst = [0.0, 0.0, 0.0]
    for gs, wd in ((1.0, 1e-2), (0.25, 0.0)):
        ref = sf.adamw_ref(p, g, m, v, t, weight_decay=wd, grad_scale=gs, **sf.HYPER)
        moved = ref["step"] != 0
        assert moved.mean() > 0.85
        share = float(np.mean(ref["bp_zero"][moved] < 1e-3 * np.abs(ref["step"][moved])))
        assert share >= 0.95, share
        pv, mv, vv = sf.adamw_f32(p, g, m, v, t, weight_decay=wd, grad_scale=gs, **sf.HYPER)
        r = sf.adamw_ratios(pv, mv, vv, ref)
        worst = [max(a, b) for a, b in zip(worst, r)]
        # a wrong exponent of the bias correction, or beta1 in place of beta2, is far outside
        if t <= 10:
            off = sf.adamw_ref(p, g, m, v, t + 1, weight_decay=wd, grad_scale=gs, **sf.HYPER)
            assert sf.adamw_ratios(off["P"], mv, vv, ref)[2] > 100
    print(f"t = {t}: float32 restatement / bound: m {worst[0]:.2f}, v {worst[1]:.2f}, p {worst[2]:.2f}")
    assert max(worst) < 1.0, worst


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("which", [0, 2, 3], ids=["p", "m", "v"])
@pytest.mark.parametrize("where", ["zero_bound", "plain"])
def test_adamw_verdict_refuses_what_is_not_finite(which, value, where):
    """One NaN or infinity in p, m or v is a failure, also at an element whose bound is zero
    (p0 = g = m0 = v0 = 0: the result must be exactly zero) and also when it sits in an array whose
    ratio is not the first one looked at: each ratio is inf there, never NaN, never skipped."""
    n, t = 1025, 3
    host = sf.adamw_inputs(n)
    ref = sf.adamw_ref(*host, t, weight_decay=0.0, **sf.HYPER)
    pv, mv, vv = sf.adamw_f32(*host, t, weight_decay=0.0, **sf.HYPER)
    good = (pv, host[1], mv, vv)
    r, problems = sf.adamw_verdict(good, host, ref)
    assert not problems and max(r.values()) < 1.0
    zero = np.nonzero((host[0] == 0) & (host[1] == 0) & (host[2] == 0) & (host[3] == 0))[0]
    assert zero.size and ref["bm"][zero[0]] == 0 and ref["bv"][zero[0]] == 0
    assert ref["bp"][zero[0]] == 0
    j = int(zero[0]) if where == "zero_bound" else n - 2
    got = [a.copy() for a in good]
    got[which][j] = value
    r, problems = sf.adamw_verdict(tuple(got), host, ref)
    name = "pgmv"[which]
    assert r[name] == np.inf and not any(np.isnan(x) for x in r.values())
    assert any(p.startswith(f"{name} is not finite") for p in problems)
    assert any(p.startswith(f"{name} is outside its bound") for p in problems)
    # the same through the ratios alone, as the old `max(r.values()) <= 1` would have read them
    ratios = sf.adamw_ratios(got[0], got[2], got[3], ref)
    assert not all(x <= 1.0 for x in ratios) and max(ratios) == np.inf


def test_adamw_verdict_refuses_a_division_by_zero_step():
    """step_size = lr / 0 (a bias correction formed from t - 1 at t = 1): p is all inf and NaN.
    The verdict fails, and so does the next step's, whose reference would start from that state."""
    n = 1025
    host = sf.adamw_inputs(n, zero_moments=True)
    ref = sf.adamw_ref(*host, 1, weight_decay=1e-2, **sf.HYPER)
    pv, mv, vv = sf.adamw_f32(*host, 1, weight_decay=1e-2, **sf.HYPER)
    with np.errstate(all="ignore"):
        broken = (pv - np.float32(np.inf) * (mv / np.float32(1.0)), host[1], mv, vv)
    assert not np.isfinite(broken[0]).any() and np.isnan(broken[0]).any()
    r, problems = sf.adamw_verdict(broken, host, ref)
    assert r["p"] == np.inf and r["m"] < 1 and r["v"] < 1 and problems
    with np.errstate(all="ignore"):
        nxt = sf.adamw_ref(*broken, 2, weight_decay=1e-2, **sf.HYPER)
        r, problems = sf.adamw_verdict(broken, broken, nxt)
    assert problems and any("starts from" in p for p in problems)
    # a step that leaves g changed is a problem too
    g2 = host[1].copy()
    g2[5] = 1.0
    assert "g was written" in sf.adamw_verdict((pv, g2, mv, vv), host, ref)[1]


def test_adamw_ref_is_torch_adamw():
    """The float64 formulas are torch.optim.AdamW's: five steps of both from one state."""
    import torch
    n = 1025
    p, g, m, v = (a.astype(np.float64) for a in sf.adamw_inputs(n, zero_moments=True))
    f = lambda x: float(np.float32(x))   # noqa: E731
    h = sf.HYPER
    tp = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=f(h["lr"]), betas=(f(h["beta1"]), f(h["beta2"])),
                            eps=f(h["eps"]), weight_decay=f(1e-2))
    for t in range(1, 6):
        gt = np.roll(g, t)
        ref = sf.adamw_ref(p, gt, m, v, t, weight_decay=1e-2, **h)
        p, m, v = ref["P"], ref["M"], ref["V"]
        tp.grad = torch.from_numpy(gt.copy())
        opt.step()
        np.testing.assert_allclose(tp.detach().numpy(), p, rtol=1e-12, atol=1e-300)
