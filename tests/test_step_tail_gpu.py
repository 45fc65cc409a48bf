"""The step's last launches against exact references, through the C ABI: l3u_reduce_segments,
l3u_reduce_segments_adamw, l3u_adamw_tick and l3u_counter_add (csrc/misc.hip segment_sum,
adamw_update, adamw_tick_kernel, reduce_segments_adamw_kernel).

A. The reduction, bit for bit.  tests/step_tail_fixture.py builds sources whose sums are exact in
   fp64 in any order ("once": every partial sum exact even in fp32; "wide": 53-bit partial sums that
   an fp32 accumulation gets wrong), NaN outside every footprint and a sentinel outside every
   output.  Hand-made lists per branch of segment_sum (float4 rows at every len / TP / batch
   boundary, the scalar form on both sides of the doubled batch, the fp64 layouts, the near-misses
   of the float4 predicate), one launch of 3000 mixed items with adjoining outputs, and every
   distinct signature of the items the engine records (traced on the CPU), accumulate 0 and 1.
B. The fused reduce + AdamW launch == l3u_reduce_segments then l3u_adamw_tick, bitwise (g, p, m, v,
   step, counter2), on every list of A and, three calls in a row per ticket buffer, at item counts
   round the 32 ticket groups; the tickets are back at zero after every call.
C. l3u_adamw_tick against torch.optim.AdamW's formulas in float64 on the fp32 state, one step at
   a time, m, v and p elementwise within the rounding bounds of step_tail_fixture.adamw_ref.
D. l3u_counter_add.

Measured on one MI355X, 2026-10-21, one pytest process: the 235 cases 4.9 s (slowest 0.32 s, the
fp64 lists), every comparison of A and B bit-equal.  l3u_adamw_tick's worst |error| / bound over
all cases of C: m 0.343, v 0.658, p 0.733 -- the figures of the float32 restatement of the kernel
on the host (tests/test_step_tail_host.py: 0.34, 0.65, 0.73), so the device's powf bias
corrections cost nothing that shows.  Fenced (tests/test_fenced_ops_gpu.py re-exports all but the
graph and the misaligned-src test): the 233 cases 12.9 s against 5.2 s unfenced.
With one scratch edit to csrc/misc.hip each (none committed; old: test_ops_gpu's
test_reduce_segments and test_adamw_tick_matches_torch as they stood):
  1 float4 batch loop drops its clamped tail     83 cases fail (every float4 list); old pass
  2 red[] summed in float                        77 fail (the wide family, the fused tests); old pass
  3 float4 predicate ignores src_off & 3         test_reduce_order_of_additions fails, nothing
                                                 else: the exact sums come out right; old pass
  4 step_size from t - 1                         83 fail: every case of C with t <= 10, those at
                                                 t = 1 (p all inf / NaN) through the verdict's
                                                 finiteness; old adamw test fails too (NaN)
  5 vv from beta1                                94 fail (every t > 1); old adamw test fails too
  6 group ticket not reset                       40 fail (ticket ints, then the step); old pass
"""
import numpy as np
import pytest
import torch

import step_tail_fixture as sf

pytestmark = pytest.mark.gpu

LISTS = sf.hand_lists()
H = sf.HYPER


def nat():
    from light_unet import _native
    return _native


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def up(a, cuda, lead=0):
    """The array, flattened, on the device, its storage starting `lead` elements before it."""
    h = torch.from_numpy(np.array(a)).reshape(-1)
    t = torch.empty(h.numel() + lead, dtype=h.dtype, device=cuda)[lead:]
    t.copy_(h)
    return t


def down(*ts):
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


# ------------------------------------------------------------------ A. l3u_reduce_segments
def run_reduce(cuda, prob):
    src, rows, dst = up(prob.src, cuda), up(prob.rows, cuda), up(prob.dst0, cuda)
    assert src.data_ptr() % 16 == 0
    nat().call("l3u_reduce_segments", src.data_ptr(), rows.data_ptr(), len(prob.rows),
               dst.data_ptr(), st())
    got = down(dst)
    assert same(down(src), prob.src)
    return got


def check(prob, got):
    assert same(got, prob.expect), sf.describe(prob, got)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("family", sf.FAMILIES)
@pytest.mark.parametrize("name", sorted(LISTS))
def test_reduce_hand_lists(cuda, name, family, acc):
    for chunk in sf.chunks(LISTS[name]):
        prob = sf.build(chunk, family, acc=acc)
        check(prob, run_reduce(cuda, prob))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("family", sf.FAMILIES)
def test_reduce_near_misses_equal_the_float4_item(cuda, family, acc):
    """An item that misses the float4 predicate by one condition (src_off 1 mod 4, istride 2 mod 4,
    len - 1) gives, through the scalar form, the reference's value and the float4 item's bits."""
    prob = sf.build(sf.near_miss_items(), family, acc=acc)
    got = run_reduce(cuda, prob)
    check(prob, got)
    k = 0
    for base, var in sf.near_miss_groups():
        do, ln = prob.outs[k]
        for j in range(1, len(var) + 1):
            dv, lv = prob.outs[k + j]
            assert same(got[dv:dv + lv], got[do:do + lv]), (base, var[j - 1])
        k += 1 + len(var)
    assert k == len(prob.outs)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("family", sf.FAMILIES)
def test_reduce_3000_mixed_items(cuda, family, acc):
    """Item indexing by workgroup: 3000 items of every form with adjoining outputs, the words
    before the first and after the last untouched."""
    prob = sf.with_margin(sf.build(sf.mixed_items(), family, acc=acc, gaps=False))
    assert len(prob.rows) == 3000
    check(prob, run_reduce(cuda, prob))


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_reduce_engine_items(cuda, family):
    """Every distinct signature of the engine's own reduction items, re-based onto a compact
    source with the same src_off mod 4."""
    items = sf.engine_items()
    assert {sf.branch(it) for it in items} == {"float4", "scalar", "scalar_long", "fp64"}
    for chunk in sf.chunks(items):
        prob = sf.build(chunk, family)
        check(prob, run_reduce(cuda, prob))


ORDER_ITEMS = (sf.near_miss_items() + sf.vec_items(32) + sf.vec_items(252) + sf.scalar_items(27)
               + sf.scalar_items(256) + sf.f64_items()[:30])


def test_reduce_order_of_additions(cuda):
    """This test pins the IMPLEMENTATION's order of additions, not the header's contract.  The
    contract is "a fixed order, a function of the item alone"; any such order satisfies it.  What
    is held here is the order segment_sum uses today: on sums that depend on the order (large terms
    that cancel, step_tail_fixture.draw_order) every item gives the bits of its own form's order
    -- thread k of TP adds the terms k, k + TP, ... in turn, the TP partial sums are added in k
    order; TP = 256 // (len // 4) for float4 rows, 256 // len otherwise.  A deliberate reordering
    of the fp64 additions in the kernel is legitimate: it changes results in the last bits from one
    build to the next, fails this test, and step_tail_fixture.order_sum is then rewritten in step.
    The test is here because it is the only way a near-miss of the float4 predicate shows which
    form it took: the hardware serves a 16-byte load from a 4-byte aligned address, so a predicate
    that forgets src_off gives the right exact sums."""
    for chunk in sf.chunks(ORDER_ITEMS):
        prob = sf.build(chunk, "order")
        check(prob, run_reduce(cuda, prob))


def test_reduce_refuses_misaligned_src(cuda):
    """include/l3u.h: src is 16-byte aligned (checked)."""
    prob = sf.build(sf.vec_items(8)[:4], "once")
    src = up(np.concatenate((prob.src[:1], prob.src)), cuda)
    rows, dst = up(prob.rows, cuda), up(prob.dst0, cuda)
    rc = nat().query("l3u_reduce_segments", src.data_ptr() + 4, rows.data_ptr(), len(prob.rows),
                     dst.data_ptr(), st())
    assert rc != 0
    assert same(down(dst), prob.dst0)
    check(prob, run_reduce(cuda, prob))     # the same launch from an aligned base


# ------------------------------------------------------------------ B. l3u_reduce_segments_adamw
class State:
    """g, p, m, v, lr, step, ticket, counter2 of one optimizer on the device."""

    def __init__(self, cuda, prob, step0, ctr0):
        n = prob.dst0.size
        p, _, m, v = sf.adamw_inputs(n)
        self.n = n
        self.g, self.p, self.m, self.v = (up(a, cuda) for a in (prob.dst0, p, m, v))
        self.lr = torch.tensor([H["lr"]], device=cuda)
        self.step = torch.tensor([step0], dtype=torch.int32, device=cuda)
        self.ticket = torch.zeros(sf.TICKET_INTS, dtype=torch.int32, device=cuda)
        self.ctr = None if ctr0 is None else torch.tensor([ctr0], dtype=torch.int32, device=cuda)

    def tail(self, wd, gs):
        return (self.lr.data_ptr(), H["beta1"], H["beta2"], H["eps"], wd, self.step.data_ptr(), gs,
                self.ticket.data_ptr(), None if self.ctr is None else self.ctr.data_ptr(), st())

    def fused(self, src, rows, wd, gs):
        nat().call("l3u_reduce_segments_adamw", src.data_ptr(), rows.data_ptr(), rows.numel() // 8,
                   self.g.data_ptr(), self.p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                   *self.tail(wd, gs))

    def two_launches(self, src, rows, wd, gs):
        nat().call("l3u_reduce_segments", src.data_ptr(), rows.data_ptr(), rows.numel() // 8,
                   self.g.data_ptr(), st())
        nat().call("l3u_adamw_tick", self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(),
                   self.v.data_ptr(), self.n, *self.tail(wd, gs))

    def read(self):
        ctr = self.step if self.ctr is None else self.ctr
        g, p, m, v, step, ticket, ctr = down(self.g, self.p, self.m, self.v, self.step, self.ticket, ctr)
        return dict(g=g, p=p, m=m, v=v, step=int(step[0]), ticket=ticket, ctr=int(ctr[0]))


def fused_vs_two(cuda, prob, calls, with_ctr, wd, gs, step0=41, ctr0=7):
    assert prob.covered().all() and not prob.rows[:, 6].any()     # the fused launch's condition
    src, rows = up(prob.src, cuda), up(prob.rows, cuda)
    a, b = (State(cuda, prob, step0, ctr0 if with_ctr else None) for _ in range(2))
    for k in range(1, calls + 1):
        a.fused(src, rows, wd, gs)
        b.two_launches(src, rows, wd, gs)
        ra, rb = a.read(), b.read()
        # the step has advanced by exactly one (a group ticket that is not reset: the second call's
        # step does not advance), counter2 too, and every ticket is back at zero
        assert ra["step"] == rb["step"] == step0 + k
        if with_ctr:
            assert ra["ctr"] == rb["ctr"] == ctr0 + k
        assert not ra["ticket"].any() and not rb["ticket"].any()
        check(prob, ra["g"])
        for key in ("g", "p", "m", "v"):
            assert same(ra[key], rb[key]), f"call {k}: {key} differs between the fused and the two launches"
        assert not same(ra["p"], sf.adamw_inputs(a.n)[0])
        assert all(np.all(np.isfinite(ra[key])) for key in ("p", "m", "v"))


@pytest.mark.parametrize("name", sorted(LISTS) + ["engine"])
def test_fused_equals_two_launches(cuda, name):
    items = sf.engine_items() if name == "engine" else LISTS[name]
    for chunk in sf.chunks(items):
        fused_vs_two(cuda, sf.build(chunk, "wide", acc=0, gaps=False), 1, True, 1e-2, 0.5)


def tickets(cuda, nitems, with_ctr):
    prob = sf.build(sf.mixed_items(nitems), "wide", acc=0, gaps=False)
    fused_vs_two(cuda, prob, 3, with_ctr, 0.0 if nitems % 2 else 1e-2, 1.0)


@pytest.mark.parametrize("with_ctr", [True, False], ids=["counter2", "no_counter2"])
@pytest.mark.parametrize("nitems", [1, 2, 31, 32, 33, 63, 64, 65])
def test_fused_tickets(cuda, nitems, with_ctr):
    """Three calls in a row on one ticket buffer, at item counts round the 32 ticket groups."""
    tickets(cuda, nitems, with_ctr)


@pytest.mark.parametrize("with_ctr", [True, False], ids=["counter2", "no_counter2"])
@pytest.mark.parametrize("nitems", [1000, 2601])
def test_fused_tickets_many_items(cuda, nitems, with_ctr):
    """The same with every ticket group taking tens of workgroups."""
    tickets(cuda, nitems, with_ctr)


# ------------------------------------------------------------------ C. l3u_adamw_tick
WORST = {"m": 0.0, "v": 0.0, "p": 0.0}


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print(f"\nl3u_adamw_tick, worst |error| / bound over this module's cases: m {WORST['m']:.3f}, "
          f"v {WORST['v']:.3f}, p {WORST['p']:.3f}")


class Tick:
    """One optimizer state on the device; lead: how many floats into its storage each of p, g, m,
    v starts (0: 16-byte aligned, the float4 path)."""

    def __init__(self, cuda, host, step0, ctr0=7, lead=(0, 0, 0, 0), lr=H["lr"]):
        self.p, self.g, self.m, self.v = (up(a, cuda, k) for a, k in zip(host, lead))
        for t, k in zip((self.p, self.g, self.m, self.v), lead):
            assert t.data_ptr() % 16 == 4 * k
        self.n = host[0].size
        self.lr = torch.tensor([lr], device=cuda)
        self.step = torch.tensor([step0], dtype=torch.int32, device=cuda)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=cuda)
        self.ctr = None if ctr0 is None else torch.tensor([ctr0], dtype=torch.int32, device=cuda)

    def call(self, wd=1e-2, gs=1.0):
        nat().call("l3u_adamw_tick", self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(),
                   self.v.data_ptr(), self.n, self.lr.data_ptr(), H["beta1"], H["beta2"], H["eps"],
                   wd, self.step.data_ptr(), gs, self.ticket.data_ptr(),
                   None if self.ctr is None else self.ctr.data_ptr(), st())

    def read(self):
        return down(self.p, self.g, self.m, self.v)

    def counters(self):
        step, ticket = down(self.step, self.ticket)
        return int(step[0]), int(ticket[0]), None if self.ctr is None else int(down(self.ctr)[0])


def within_bounds(got, host, t, what, lr=H["lr"], wd=1e-2, gs=1.0):
    """got = (p, g, m, v) after step t from host = (p0, g, m0, v0)."""
    ref = sf.adamw_ref(*host, t, lr, H["beta1"], H["beta2"], H["eps"], wd, gs)
    r, problems = sf.adamw_verdict(got, host, ref)
    print(f"{what}: |error| / bound m {r['m']:.3f}, v {r['v']:.3f}, p {r['p']:.3f}")
    # (a result that is not finite is a ratio of inf and a problem of its own: never skipped)
    assert not problems, f"{what}: {'; '.join(problems)}"
    for k in r:
        WORST[k] = max(WORST[k], r[k])
    return ref


def one_step(cuda, n, t, wd=1e-2, gs=1.0, ctr0=7, lead=(0, 0, 0, 0)):
    host = sf.adamw_inputs(n, zero_moments=(t == 1))
    s = Tick(cuda, host, t - 1, ctr0, lead)
    s.call(wd, gs)
    got = s.read()
    assert s.counters() == (t, 0, None if ctr0 is None else ctr0 + 1)
    return host, got


@pytest.mark.parametrize("n", sf.ADAMW_SIZES)
@pytest.mark.parametrize("t", sf.ADAMW_STEPS)
def test_adamw_one_step(cuda, t, n):
    """Step t (from a preset *step) at every size: the 1-3 element tail, one and several
    workgroups, the capped grid with more than one stride iteration plus the tail."""
    host, got = one_step(cuda, n, t)
    within_bounds(got, host, t, f"t {t}, numel {n}")


@pytest.mark.parametrize("n", [5, 1025, 217229])
@pytest.mark.parametrize("which", range(4), ids=["p", "g", "m", "v"])
def test_adamw_scalar_path_equals_float4_path(cuda, which, n):
    """One of p, g, m, v one float into its storage selects the scalar path: the same bits."""
    host, want = one_step(cuda, n, 10)
    lead = tuple(int(k == which) for k in range(4))
    _, got = one_step(cuda, n, 10, lead=lead)
    for name, a, b in zip("pgmv", got, want):
        assert same(a, b), f"{name} differs between the scalar and the float4 path"
    within_bounds(got, host, 10, f"scalar path ({'pgmv'[which]} + 4 bytes), numel {n}")


@pytest.mark.parametrize("n", [1025, 217229])
@pytest.mark.parametrize("with_ctr", [True, False], ids=["counter2", "no_counter2"])
@pytest.mark.parametrize("wd", [1e-2, 0.0])
@pytest.mark.parametrize("gs", [1.0, 0.5, 0.25])
def test_adamw_options(cuda, gs, wd, with_ctr, n):
    host, got = one_step(cuda, n, 3, wd=wd, gs=gs, ctr0=7 if with_ctr else None)
    within_bounds(got, host, 3, f"grad_scale {gs}, weight_decay {wd}, numel {n}", wd=wd, gs=gs)
    if wd == 0.0:     # no decay: a parameter whose step is zero keeps its bits
        ref = sf.adamw_ref(*host, 3, weight_decay=0.0, grad_scale=gs, **H)
        still = ref["step"] == 0
        assert still.any() and same(got[0][still], host[0][still])


def test_adamw_lr_rewritten_on_the_device(cuda):
    """What FlatAdamW.set_lr relies on: lr is read from the device at every call; no host
    argument changes between the two calls."""
    n = 1025
    host = sf.adamw_inputs(n, zero_moments=True)
    s = Tick(cuda, host, 0, lr=1e-3)
    s.call()
    mid = s.read()
    within_bounds(mid, host, 1, "lr 1e-3, step 1", lr=1e-3)
    s.lr.fill_(3e-4)
    s.call()
    got = s.read()
    assert s.counters() == (2, 0, 9)
    within_bounds(got, mid, 2, "lr 3e-4 written on the device, step 2", lr=3e-4)
    stale = sf.adamw_ref(*mid, 2, weight_decay=1e-2, **dict(H, lr=1e-3))
    assert sf.adamw_ratios(got[0], got[2], got[3], stale)[2] > 100     # the old lr is far outside


@pytest.mark.parametrize("n", [1025, 217229])
def test_adamw_five_steps(cuda, n):
    """Five consecutive steps from zero moments, the reference restarted from the device's fp32
    state at every step (errors do not compound into the bound)."""
    p0, g0, m0, v0 = sf.adamw_inputs(n, zero_moments=True)
    s = Tick(cuda, (p0, g0, m0, v0), 0)
    state = (p0, g0, m0, v0)
    for t in range(1, 6):
        g = np.roll(g0, 13 * t)
        s.g.copy_(torch.from_numpy(g))
        state = (state[0], g, state[2], state[3])
        s.call()
        got = s.read()
        assert s.counters() == (t, 0, 7 + t)
        within_bounds(got, state, t, f"step {t} of five, numel {n}")
        state = got


def test_adamw_graph_replay_equals_eager(cuda):
    """One captured single-stream graph of one call, replayed three times with lr changed between
    the replays: step and counter2 advance per replay, the results are the eager calls' bits."""
    n = 217229
    host = sf.adamw_inputs(n)
    lrs = (1e-3, 5e-4, 2e-3)
    eager, e = [], Tick(cuda, host, 9)
    for lr in lrs:
        e.lr.fill_(lr)
        e.call()
        eager.append((e.read(), e.counters()))
    s = Tick(cuda, host, 9)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.call()
    torch.cuda.synchronize()
    assert s.counters() == (9, 0, 7) and same(s.read()[0], host[0])    # captured, not run
    for k, lr in enumerate(lrs):
        s.lr.fill_(lr)
        graph.replay()
        got, counters = s.read(), s.counters()
        assert counters == eager[k][1] == (10 + k, 0, 8 + k)
        for name, a, b in zip("pgmv", got, eager[k][0]):
            assert same(a, b), f"replay {k}: {name} differs from the eager call"


# ------------------------------------------------------------------ D. l3u_counter_add
def test_counter_add(cuda):
    c = torch.tensor([5, -77], dtype=torch.int32, device=cuda)
    want = 5
    for v in (3, 3, -10, -10, 2 ** 20, -2 ** 20):
        nat().call("l3u_counter_add", c.data_ptr(), v, st())
        want += v
        assert down(c).tolist() == [want, -77]
