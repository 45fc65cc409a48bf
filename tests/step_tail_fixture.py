"""Inputs, exact references and error bounds for the step's last launches: the segmented reduction
(csrc/misc.hip segment_sum) and the AdamW update (adamw_update), shared by
tests/test_step_tail_host.py and tests/test_step_tail_gpu.py.  numpy on the host, no device.

The reduction.  include/l3u.h: dst[dst_off + t] (+)= fl32(fp64 sum over i < count of
src[src_off + i*istride + t*tstride]).  The inputs are integers times a power of two, small
enough that every partial sum of an item (and the prior dst of an accumulating one) is exact in
fp64 IN ANY ORDER, so the expected value is an integer sum rounded once to fp32 and the
comparison is bit for bit:
  "once"  non-zero integers, |x| <= 2^11 and (count + 1) * |x| <= 2^24: every partial sum is exact
          even in fp32, so only a dropped, repeated or misplaced term changes the bits;
  "wide"  fp32 sources: +-m * 2^e * 2^-30, m a full 24-bit integer, e in [0, 18] and
          (count + 1) * 2^(24 + e) <= 2^53 (e <= 18 up to 1024 terms, one less per doubling of the
          list); fp64 sources: integers below 2^40, (count + 1) * |x| < 2^53.  Every partial sum
          fits 53 bits, an fp32 accumulation (or an fp32 rounding before the last combine) does
          not reproduce it.
A third family, "order", is the opposite: sums that depend on the order of the fp64 additions
(draw_order), whose expected bits are those of segment_sum's own order for the item's form
(order_sum).  It pins that order, and with it which form an item took.
`build` lays a list of items out on one compact source: every word outside an item's own footprint
is NaN (the gaps of a strided footprint, the space between items), every dst word outside the
items' outputs carries SENTINEL, and a non-accumulating output starts as SENTINEL too.

The update.  `adamw_ref` is torch.optim.AdamW in float64 on the fp32 state and the float-rounded
hyper-parameters, with elementwise bounds that count the kernel's fp32 roundings (stated there);
`adamw_inputs` are built so that the step itself is visible; `adamw_f32` restates the kernel in
numpy float32 so that the host can check the bounds leave it room.
"""
import collections
import importlib.util
import os

import numpy as np

from footprints import TICKET_INTS  # noqa: F401  (include/l3u.h L3U_ADAMW_TICKET_INTS, kept there)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# csrc/misc.hip
SEG_BATCH, SEG_LONG = 8, 32
SENTINEL = 0x7FA51C3D          # a NaN with a payload: compared as bits
MAX_WORDS = 4 << 20            # one source buffer: 16 MB of fp32 words
FAMILIES = ("once", "wide")
U32 = 2.0 ** -24

Item = collections.namedtuple("Item", "count istride tstride len acc f64 mod seed cols")


def item(count, istride, tstride, ln, acc=0, f64=0, mod=0, seed=None, cols=None):
    """One reduction item without its addresses.  mod: src_off modulo 4; seed / cols: items with
    the same seed, count and cols draw the same count x cols values and use their first len
    columns (the near-miss groups)."""
    return Item(count, istride, tstride, ln, acc, f64, mod, seed, cols or ln)


# ------------------------------------------------------------------ segment_sum's dispatch
def is_vec(it):
    return (not it.f64 and it.tstride == 1 and it.len % 4 == 0 and it.istride % 4 == 0
            and it.mod % 4 == 0)


def tp(it):
    """Threads per output."""
    return 256 // (it.len // 4) if is_vec(it) else 256 // it.len


def branch(it):
    if is_vec(it):
        return "float4"
    if it.f64:
        return "fp64"
    return "scalar_long" if it.count > SEG_LONG * tp(it) else "scalar"


def signature(it):
    return (it.count, it.istride, it.tstride, it.len, it.acc, it.f64, it.mod)


def span(it):
    """Elements (of the item's own type) from its first to its last source element."""
    return (it.count - 1) * it.istride + (it.len - 1) * it.tstride + 1


def words(it):
    return span(it) * (2 if it.f64 else 1)


# ------------------------------------------------------------------ the two input families
def draw(rng, family, f64, shape, count, fp32_exact=False):
    """(q int64, scale): the values are q * scale.  count: the terms of the sum the values take
    part in (the bounds leave room for one more, the prior dst).  fp32_exact: representable in
    fp32 although the source is fp64 (a prior dst)."""
    sign = 1 - 2 * rng.integers(0, 2, shape, dtype=np.int64)
    bl = int(count).bit_length()          # count + 1 <= 2^bl
    if family == "once":
        xmax = min(2 ** 11, 2 ** 24 // (count + 1))
        assert xmax >= 1
        return sign * rng.integers(1, xmax + 1, shape, dtype=np.int64), 1.0
    assert family == "wide"
    if not f64:
        emax = min(18, 29 - bl)
        assert emax >= 0
        m = rng.integers(2 ** 23, 2 ** 24, shape, dtype=np.int64)
        return sign * (m << rng.integers(0, emax + 1, shape, dtype=np.int64)), 2.0 ** -30
    bits = min(40, 53 - bl)
    if fp32_exact:
        m = rng.integers(2 ** 23, 2 ** 24, shape, dtype=np.int64)
        return sign * (m << rng.integers(0, bits - 24 + 1, shape, dtype=np.int64)), 1.0
    return sign * rng.integers(1, 2 ** bits, shape, dtype=np.int64), 1.0


def draw_order(rng, shape):
    """Values whose fp64 sum DEPENDS on the order: per output a third of the terms are large
    (+-m * 2^e, e in [20, 60]), a third their negations, the rest small (e in [-30, 0]), shuffled.
    The exact sum is the small terms'; what a given order of fp64 additions leaves is rounding
    noise of the large ones, different for every order and the same bits for the same one."""
    cnt, ln = shape
    mant = lambda: ((1 - 2 * rng.integers(0, 2, shape)) * rng.integers(2 ** 23, 2 ** 24, shape)).astype(np.float64)  # noqa: E731
    x = mant() * 2.0 ** rng.integers(-30, 1, shape)
    big = mant() * 2.0 ** rng.integers(20, 61, shape)
    h = cnt // 3
    order = np.argsort(rng.random(shape), axis=0)
    np.put_along_axis(x, order[:h], big[:h], axis=0)
    np.put_along_axis(x, order[h:2 * h], -big[:h], axis=0)
    return x


def order_sum(x, t):
    """segment_sum's order of additions on x[count][len] with t threads per output, in fp64:
    thread k adds the terms k, k + t, k + 2t, ... one after the other from 0, then the t partial
    sums are added in k order from 0.  (The batches of 8 or 16 loads in flight add in the same
    order; a slot past the end adds +0.0.)  This restates the implementation, not the header's
    contract (any fixed order would meet that): a kernel change that reorders the additions on
    purpose rewrites this function with it."""
    x = np.asarray(x, dtype=np.float64)
    part = np.zeros((t, x.shape[1]))
    for i0 in range(0, x.shape[0], t):
        blk = x[i0:i0 + t]
        part[:blk.shape[0]] += blk
    r = np.zeros(x.shape[1])
    for k in range(t):
        r = r + part[k]
    return r


def to_f32(total, scale):
    """fl32 of the integer totals (|total| < 2^53: the int64 -> fp64 step and the power-of-two
    scale are exact, the cast rounds once, to nearest even)."""
    assert np.all(np.abs(total) < 2 ** 53)
    return (total.astype(np.float64) * scale).astype(np.float32)


class Problem:
    """One launch: src (fp32 words, fp64 items inside), rows (int64 [n][8]), dst0 and expect
    (fp32, compared as int32 bits), outs [(dst_off, len)] per item."""

    def __init__(self, items, src, rows, dst0, expect, qs):
        self.items, self.src, self.rows, self.dst0, self.expect, self.qs = \
            items, src, rows, dst0, expect, qs
        self.outs = [(int(r[5]), int(r[4])) for r in rows]

    def covered(self):
        """The dst elements some item writes."""
        m = np.zeros(self.dst0.size, dtype=bool)
        for do, ln in self.outs:
            m[do:do + ln] = True
        return m


def _up(v, k):
    return -(-v // k) * k


def build(items, family, acc=None, gaps=True, keep=False):
    """Lay `items` out on a compact source and dst.  acc: 0 / 1 overrides every item's flag, None
    keeps it.  gaps: SENTINEL words round every item's outputs; False: adjoining outputs from
    dst_off 0 (every element written exactly once: the fused launch's condition).  keep: also the
    integers of every item ([count][len]) and of its prior dst, for the host's self-check."""
    fam = (FAMILIES + ("order",)).index(family)
    items = [it if acc is None else it._replace(acc=acc) for it in items]
    pos, dpos, place = 4, (1 if gaps else 0), []
    for k, it in enumerate(items):
        if it.f64:
            so = _up((pos + 2) // 2, 4) + it.mod       # in doubles from the same base
            pos = 2 * (so + span(it))
        else:
            so = _up(pos + 1, 4) + it.mod
            pos = so + span(it)
        place.append((so, dpos))
        dpos += it.len + ((1 + k % 3) if gaps else 0)
    src = np.full(_up(pos + 4, 4), np.nan, dtype=np.float32)
    src64 = src.view(np.float64)
    dst0 = np.full(dpos, SENTINEL, dtype=np.int32).view(np.float32)
    expect = dst0.copy()
    rows = np.zeros((len(items), 8), dtype=np.int64)
    qs = []
    for k, (it, (so, do)) in enumerate(zip(items, place)):
        rng = np.random.default_rng([fam, it.seed if it.seed is not None else 1000 + k])
        idx = (so + np.arange(it.count, dtype=np.int64)[:, None] * it.istride
               + np.arange(it.len, dtype=np.int64)[None, :] * it.tstride)
        rows[k] = (so, it.count, it.istride, it.tstride, it.len, do, it.acc, it.f64)
        if family == "order":
            # order-dependent sums: the expected bits are those of the item's own form
            assert not it.acc
            x = draw_order(rng, (it.count, it.cols))[:, :it.len]
            if it.f64:
                src64[so:so + span(it)] = np.nan
                src64[idx] = x
            else:
                src[idx] = x.astype(np.float32)
                assert np.array_equal(src[idx].astype(np.float64), x)
            expect[do:do + it.len] = order_sum(x, tp(it)).astype(np.float32)
            if keep:
                qs.append((x, None, None))
            continue
        q, scale = draw(rng, family, it.f64, (it.count, it.cols), it.count)
        q = q[:, :it.len]
        if it.f64:
            src64[so:so + span(it)] = np.nan
            src64[idx] = q.astype(np.float64) * scale
        else:
            src[idx] = (q.astype(np.float64) * scale).astype(np.float32)
        total, prior = q.sum(axis=0), None
        if it.acc:
            prior, pscale = draw(rng, family, it.f64, (it.cols,), it.count, fp32_exact=True)
            assert pscale == scale
            prior = prior[:it.len]
            dst0[do:do + it.len] = to_f32(prior, scale)
            total = total + prior
        expect[do:do + it.len] = to_f32(total, scale)
        if keep:
            qs.append((q, prior, scale))
    return Problem(items, src, rows, dst0, expect, qs)


def with_margin(prob, k=8):
    """prob with k SENTINEL words before and after its dst (an adjoining layout's neighbours)."""
    pad = np.full(k, SENTINEL, dtype=np.int32).view(np.float32)
    rows = prob.rows.copy()
    rows[:, 5] += k
    return Problem(prob.items, prob.src, rows, np.concatenate((pad, prob.dst0, pad)),
                   np.concatenate((pad, prob.expect, pad)), prob.qs)


def chunks(items, max_words=MAX_WORDS):
    """`items` in order, split so that no chunk's source exceeds max_words."""
    out, cur, n = [], [], 0
    for it in items:
        w = words(it) + 8
        assert w <= max_words, it
        if cur and n + w > max_words:
            out.append(cur)
            cur, n = [], 0
        cur.append(it)
        n += w
    if cur:
        out.append(cur)
    return out


def describe(prob, got):
    """Where `got` (fp32 array) first differs from prob.expect, for an assertion message."""
    bad = np.nonzero(got.view(np.int32) != prob.expect.view(np.int32))[0]
    if bad.size == 0:
        return "equal"
    j = int(bad[0])
    owner = [k for k, (do, ln) in enumerate(prob.outs) if do <= j < do + ln]
    what = "outside every item's outputs"
    if owner:
        k = owner[0]
        what = (f"output {j - prob.outs[k][0]} of item {k} {tuple(int(v) for v in prob.rows[k])} "
                f"({branch(prob.items[k])}, TP {tp(prob.items[k])})")
    word = lambda a: int(a.view(np.int32)[j]) & 0xFFFFFFFF   # noqa: E731
    return (f"{bad.size} of {got.size} dst words differ; first at dst[{j}], {what}: got "
            f"{float(got[j])!r} ({word(got):#010x}), expected {float(prob.expect[j])!r} "
            f"({word(prob.expect):#010x})")


# ------------------------------------------------------------------ hand-made item lists
VEC_LENS = (4, 8, 12, 20, 32, 64, 100, 128, 252, 256)
SCALAR_LENS = (1, 3, 5, 27, 100, 255, 256)


def _counts(vals):
    return sorted({int(c) for c in vals if c > 0})


def vec_items(ln):
    """float4 form: tstride 1, len, istride and src_off multiples of 4."""
    t = 256 // (ln // 4)
    out = []
    for c in _counts((1, t - 1, t, t + 1, 8 * t - 1, 8 * t, 8 * t + 1, 864, 1728)):
        out += [item(c, ln, 1, ln), item(c, ln + 12, 1, ln)]
    assert all(branch(it) == "float4" for it in out)
    return out


def scalar_items(ln):
    """Scalar fp32 form: contiguous rows that miss the float4 predicate (istride len + 1, src_off
    1 mod 4), three interleaved columns (tstride 3), and the norm-gradient layout (istride 3,
    tstride count * 3); counts round TP, the 8- and 16-deep batches and the kSegLong threshold."""
    t = 256 // ln
    cs = _counts((1, t - 1, t, t + 1, 8 * t - 1, 8 * t, 8 * t + 1, 16 * t - 1, 16 * t, 16 * t + 1,
                  SEG_LONG * t - 1, SEG_LONG * t, SEG_LONG * t + 1, 48 * t - 1, 48 * t, 48 * t + 1))
    out = []
    for c in cs:
        out += [item(c, ln + 1, 1, ln, mod=1), item(c, 3 * ln + 1, 3, ln, mod=2),
                item(c, 3, 3 * c, ln, mod=3)]
    assert {branch(it) for it in out} == {"scalar", "scalar_long"}
    return out


def f64_items():
    """fp64 form in the engine's layouts: rows of c0 + 1 doubles read as len c0 and as the last
    column alone, and istride 2 / 3 with tstride count * istride."""
    out = []
    for c in (1, 7, 8, 9, 108, 864, 4096):
        for c0 in (8, 16, 128):
            out += [item(c, c0 + 1, 1, c0, f64=1), item(c, c0 + 1, 1, 1, f64=1, mod=c0 % 4)]
        for ist in (2, 3):
            for ln in (8, 64, 256):
                if c * ln <= 2 ** 16:      # (the source stays small)
                    out.append(item(c, ist, c * ist, ln, f64=1, mod=c % 3))
    assert all(branch(it) == "fp64" for it in out)
    return out


def near_miss_groups():
    """[(float4 item, [variants])]: src_off 1 mod 4, istride 2 mod 4, len - 1.  A group shares its
    values, so every variant's outputs are the float4 item's (its first len - 1 for the last)."""
    out = []
    for g, (ln, c) in enumerate(((32, 864), (8, 257), (256, 33), (100, 81), (4, 2049), (12, 1))):
        kw = dict(seed=500 + g, cols=ln)
        base = item(c, ln + 12, 1, ln, **kw)
        var = [item(c, ln + 12, 1, ln, mod=1, **kw), item(c, ln + 14, 1, ln, **kw),
               item(c, ln + 12, 1, ln - 1, **kw)]
        assert branch(base) == "float4" and all(branch(v) != "float4" for v in var)
        out.append((base, var))
    return out


def near_miss_items():
    return [it for base, var in near_miss_groups() for it in [base] + var]


def hand_lists():
    """{name: [Item]} of every hand-made list, each within one source buffer."""
    out = {f"vec{ln}": vec_items(ln) for ln in VEC_LENS}
    out.update({f"scalar{ln}": scalar_items(ln) for ln in SCALAR_LENS})
    out["f64"] = f64_items()
    out["near_miss"] = near_miss_items()
    return out


_CACHE = {}


def mixed_items(n=3000):
    """n items of every form drawn from the hand-made lists (those of at most 2048 source words;
    8500 for the doubled-batch scalar form, whose shortest lists are longer), in a fixed shuffled
    order: item indexing by workgroup, adjoining outputs."""
    if "pool" not in _CACHE:
        _CACHE["pool"] = [it for name, its in hand_lists().items() if name != "near_miss"
                          for it in its
                          if words(it) <= (8500 if branch(it) == "scalar_long" else 2048)]
    pool = _CACHE["pool"]
    pick = np.random.default_rng(3000).integers(0, len(pool), 3000)
    return [pool[int(k)] for k in pick[:n]]


# ------------------------------------------------------------------ the engine's own items
ENGINE_CASES = ("c16_48", "c16_n2_32", "c8_12x20x16", "c8_16_grouped")
BENCH_SHAPE = (4, 48, 48, 48)


def engine_items():
    """One Item per distinct signature (count, istride, tstride, len, accumulate, f64, src_off mod
    4) of the reduction items the engine records for ENGINE_CASES and the benchmarked batch, traced
    on the CPU (tools/launch_trace.trace_raw)."""
    if "engine" not in _CACHE:
        spec = importlib.util.spec_from_file_location(
            "launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
        lt = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(lt)
        cases = [c for c in lt.cases() if c.name in ENGINE_CASES]
        assert len(cases) == len(ENGINE_CASES)
        cases.append(lt.Case("c16_b4_48", lt.BIG, BENCH_SHAPE, opt=True))
        sigs = set()
        for c in cases:
            _, labelled, _ = lt.trace_raw(c)
            for so, cnt, ist, tst, ln, _, acc, f64 in labelled["items"].tolist():
                sigs.add((cnt, ist, tst, ln, acc, f64, so % 4))
        _CACHE["engine"] = [item(c, i, t, ln, acc=a, f64=f, mod=m) for c, i, t, ln, a, f, m in sorted(sigs)]
    return _CACHE["engine"]


# ------------------------------------------------------------------ AdamW
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
ADAMW_STEPS = (1, 2, 3, 10, 1000, 100000)
ADAMW_SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1025, 217228 + 1, 2 * 2 ** 20 + 5)


def adamw_inputs(n, zero_moments=False, seed=0):
    """(p, g, m, v) fp32: the first half of p exactly zero (the step itself is visible, not hidden
    under u|p|), |g| log-uniform over six decades (none below 2^-40: no denormal intermediate),
    every 11th g zero, every 7th m and v zero."""
    key = (n, zero_moments, seed)
    if key not in _CACHE:
        rng = np.random.default_rng([77, seed, n])
        sgn = lambda: 1.0 - 2.0 * rng.integers(0, 2, n)   # noqa: E731
        p = rng.standard_normal(n)
        p[:(n + 1) // 2] = 0.0
        g = sgn() * 10.0 ** rng.uniform(-6.0, 0.0, n)
        m = sgn() * 10.0 ** rng.uniform(-6.0, 0.0, n)
        v = 10.0 ** rng.uniform(-12.0, 0.0, n)
        i = np.arange(n)
        g[i % 11 == 10] = 0.0
        m[i % 7 == 6] = 0.0
        v[i % 7 == 6] = 0.0
        if zero_moments:
            m[:], v[:] = 0.0, 0.0
        out = tuple(a.astype(np.float32) for a in (p, g, m, v))
        assert not np.any((out[1] != 0) & (np.abs(out[1]) < 2.0 ** -40))
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def adamw_ref(p0, g, m0, v0, t, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    """torch.optim.AdamW's step number t (>= 1) in float64 on the fp32 state and on the hyper-
    parameters as the kernel receives them (rounded to float, widened): only the kernel's own
    arithmetic is under test.  Returns M, V, P, the step SS*U and the elementwise bounds

      |m - M| <= 3u (|M0| + |G|)                       u = 2^-24, G = g * grad_scale
      |v - V| <= 3u (|V0| + G^2)
      |p - P| <= SS [(2u/BC1 + u/BC2 + 8u) |U| + 4u (|M0| + |G|) / DEN] + 2u |P0| + u |P|

    BC1 = 1 - beta1^t, BC2 = 1 - beta2^t, SS = lr / BC1, DEN = sqrt(V) / sqrt(BC2) + eps,
    U = M / DEN: the fp32 roundings of adamw_update, one ulp of 1 on each bias correction formed
    in fp32, and the cancellation in m."""
    f = lambda x: float(np.float32(x))   # noqa: E731
    lr, b1, b2, eps, wd, gs = f(lr), f(beta1), f(beta2), f(eps), f(weight_decay), f(grad_scale)
    P0, G, M0, V0 = (np.asarray(a, dtype=np.float64) for a in (p0, g, m0, v0))
    G = G * gs
    M = M0 + (1.0 - b1) * (G - M0)
    V = V0 * b2 + (1.0 - b2) * G * G
    BC1, BC2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    SS = lr / BC1
    DEN = np.sqrt(V) / np.sqrt(BC2) + eps
    Uq = M / DEN
    P = P0 * (1.0 - lr * wd) - SS * Uq
    u = U32
    bm = 3 * u * (np.abs(M0) + np.abs(G))
    bv = 3 * u * (np.abs(V0) + G * G)
    bstep = SS * ((2 * u / BC1 + u / BC2 + 8 * u) * np.abs(Uq) + 4 * u * (np.abs(M0) + np.abs(G)) / DEN)
    bp = bstep + 2 * u * np.abs(P0) + u * np.abs(P)
    return dict(M=M, V=V, P=P, step=SS * Uq, bm=bm, bv=bv, bp=bp,
                bp_zero=bstep + u * np.abs(SS * Uq))


def adamw_ratios(p, m, v, ref):
    """max over the elements of |error| / bound for (m, v, p), never NaN.  An element whose bound
    is 0 must be exact (it counts as 0, or as inf when it is not); a result that is not finite, or
    an error or ratio that is not a number, counts as inf, so that it is outside every bound."""
    out = []
    for got, want, bound in ((m, ref["M"], ref["bm"]), (v, ref["V"], ref["bv"]), (p, ref["P"], ref["bp"])):
        got = np.asarray(got, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.abs(got - want)
            r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        r = np.where(np.isfinite(got) & np.isfinite(r), r, np.inf)
        out.append(float(r.max()))
    assert not any(np.isnan(x) for x in out)
    return tuple(out)


def adamw_verdict(got, host, ref):
    """(ratios {m, v, p}, problems): got = (p, g, m, v) after the step that ref describes, from
    host = (p0, g, m0, v0).  problems is empty when the state the reference starts from is finite,
    p, m and v are finite, g is untouched and EACH of the three ratios is at most 1."""
    bad = [f"the reference starts from a {n}0 that is not finite" for n, a in zip("pgmv", host)
           if not np.all(np.isfinite(a))]
    for n, a in (("p", got[0]), ("m", got[2]), ("v", got[3])):
        k = int(np.sum(~np.isfinite(np.asarray(a))))
        if k:
            bad.append(f"{n} is not finite on {k} of {np.asarray(a).size} elements")
    if not np.array_equal(np.ascontiguousarray(got[1]).view(np.int32),
                          np.ascontiguousarray(host[1]).view(np.int32)):
        bad.append("g was written")
    r = dict(zip("mvp", adamw_ratios(got[0], got[2], got[3], ref)))
    bad += [f"{n} is outside its bound: |error| / bound {x:.3g}" for n, x in r.items() if not x <= 1.0]
    return r, bad


def adamw_f32(p0, g, m0, v0, t, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    """csrc/misc.hip adamw_step + adamw_update restated in numpy float32 (no FMA), for the host's
    check that the bounds leave the kernel room."""
    f = np.float32
    lr, b1, b2, eps, wd, gs = f(lr), f(beta1), f(beta2), f(eps), f(weight_decay), f(grad_scale)
    one = f(1.0)
    bc1 = one - f(np.power(b1, f(t)))
    bc2s = np.sqrt(one - f(np.power(b2, f(t))))
    ss, decay = lr / bc1, one - lr * wd
    gv = g.astype(f) * gs
    pv = p0.astype(f) * decay
    mv = m0 + (one - b1) * (gv - m0)
    vv = v0 * b2 + (one - b2) * gv * gv
    den = np.sqrt(vv) / bc2s + eps
    pv = pv - ss * (mv / den)
    assert pv.dtype == mv.dtype == vv.dtype == np.float32
    return pv, mv, vv
