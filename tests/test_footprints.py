"""CPU: the footprint table (tests/footprints.py) against the engine's launch plan.

Completeness: every launch entry point engine.py names, and every one a traced case calls, has a
table entry (no allow-list).  Then the 45 traced configurations of tools/launch_trace.py, call by
call, on the raw events with their live CPU addresses:
  - every footprint lies inside the one labelled buffer its pointer falls in (a host query that
    promises less than the table's layout, or an arena region laid out too short, fails here);
  - no written footprint overlaps another operand's footprint of the same call, except the pairs
    the table marks as in-place;
  - every footprint read inside an arena is covered by footprints written by earlier calls of the
    same two-step trace: no launch reads a partial that no launch produced.
Static: every "l3u_..." literal of the modules tests/test_fenced_ops_gpu.py re-exports is a host
query, has a table entry, or is listed there as "end guards only".
The check is itself checked on planted faults (an under-promising query, an unwritten partial).
Needs the built library (its host queries), no GPU.
"""
import bisect
import importlib.util
import os
import re

import numpy as np
import pytest

import footprints as fp
from light_unet import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARENAS = ("fwd_arena", "bwd_arena")
FENCED_SOURCES = ("test_ops_gpu", "test_tail_bwd_gpu", "test_dwpw_gpu", "test_gconv_gpu",
                  "test_bf16_gpu", "test_loss_family_gpu", "test_step_tail_gpu")


@pytest.fixture(scope="module")
def lt():
    spec = importlib.util.spec_from_file_location(
        "launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mask(ivs, lo0, n):
    """bool[n] over 4-byte words from byte lo0: the words the byte intervals touch."""
    d = np.zeros(n + 1, dtype=np.int32)
    lo = (np.array([i[0] for i in ivs], dtype=np.int64) - lo0) // 4
    hi = (np.array([i[1] for i in ivs], dtype=np.int64) - lo0 + 3) // 4
    np.add.at(d, lo, 1)
    np.add.at(d, hi, -1)
    return np.cumsum(d[:-1]) > 0


def check_case(lt, case):
    """(problems, names called, calls checked) of one traced configuration."""
    events, labelled, _ = lt.trace_raw(case)
    canon = lt.Canon(labelled)
    starts = canon.starts
    items = labelled.get("items")

    def items_of(ptr, n):
        assert items is not None and ptr == items.data_ptr() and n == items.shape[0]
        return items.tolist()

    written = {}
    for name in ARENAS:
        if name in labelled:
            t = labelled[name]
            assert t.data_ptr() % 4 == 0
            written[name] = np.zeros(t.numel() * t.element_size() // 4, dtype=bool)
    bad, called, ncalls = [], set(), 0

    def report(ev, msg):
        bad.append(f"{case.name}: {canon.event(ev)}\n    {msg}")

    for ev in events:
        if ev[0] != "call":
            continue
        name, args = ev[1], ev[2]
        called.add(name)
        ncalls += 1
        ops = fp.footprints(name, args, items_of)
        if ops is None:
            report(ev, "no footprint entry")
            continue
        allowed = fp.inplace_pairs(name)
        declared = {o.arg for o in ops}
        for i, a in enumerate(args[:-1]):
            if nat._SIGS[name][i] is nat.P and a is not None and i not in declared:
                report(ev, f"pointer argument {i} has no footprint declaration")
        per_buf = {}
        for o in ops:
            if not o.ivs:
                continue
            k = bisect.bisect_right(starts, o.ptr) - 1
            if k < 0 or o.ptr >= canon.table[k][1]:
                report(ev, f"argument {o.arg} {o.field or ''}: {o.ptr:#x} in no labelled buffer")
                continue
            blo, bhi, label = canon.table[k]
            lo, hi = o.ptr + o.ivs[0][0], o.ptr + o.ivs[-1][1]
            if lo < blo or hi > bhi:
                report(ev, f"argument {o.arg} {o.field or ''} ({o.role}): footprint "
                           f"[{lo - blo}, {hi - blo}) leaves {label} of {bhi - blo} bytes")
                continue
            per_buf.setdefault(label, []).append((o, blo))
        # written footprints against every other operand of the call
        for label, lst in per_buf.items():
            if len({(o.arg, o.field) for o, _ in lst}) < 2:
                continue
            flat = sorted((o.ptr + a, o.ptr + b, o) for o, _ in lst for a, b in o.ivs)
            for (alo, ahi, oa), (blo_, bhi_, ob) in zip(flat, flat[1:]):
                if blo_ < ahi and (oa.arg, oa.field) != (ob.arg, ob.field) \
                        and "w" in oa.role + ob.role \
                        and frozenset((oa.arg, ob.arg)) not in allowed:
                    report(ev, f"arguments {oa.arg} ({oa.role}) and {ob.arg} ({ob.role}) overlap "
                               f"in {label} at byte {blo_ - lst[0][1]}")
                    break
        # reads of arena memory are covered by earlier writes; then this call's writes count
        for label in ARENAS:
            lst = per_buf.get(label, [])
            if not lst:
                continue
            base = lst[0][1]
            span_lo = min(o.ptr + o.ivs[0][0] for o, _ in lst) - base
            span_hi = max(o.ptr + o.ivs[-1][1] for o, _ in lst) - base
            w0, n = span_lo // 4, (span_hi + 3) // 4 - span_lo // 4
            seen = written[label][w0:w0 + n]
            marks = []
            for o, _ in lst:
                m = _mask([(o.ptr - base + a, o.ptr - base + b) for a, b in o.ivs], 4 * w0, n)
                if "r" in o.role:
                    miss = np.flatnonzero(m & ~seen)
                    if miss.size:
                        report(ev, f"argument {o.arg} {o.field or ''} reads {label}+"
                                   f"{4 * (w0 + int(miss[0]))} ({miss.size} words in all) that no "
                                   "earlier call wrote")
                if "w" in o.role:
                    marks.append(m)
            for m in marks:
                seen |= m
    return bad, called, ncalls


@pytest.fixture(scope="module")
def checked(lt):
    """One pass over every traced configuration (the tensors of a case are freed before the next)."""
    bad, called, ncalls = {}, set(), 0
    for case in lt.cases():
        b, c, n = check_case(lt, case)
        bad[case.name] = b
        called |= c
        ncalls += n
    return bad, called, ncalls


def test_every_engine_entry_point_has_a_footprint(lt):
    missing = sorted(n for n in lt.engine_entry_points() if not fp.has_entry(n))
    assert not missing, f"no footprint entry for {missing}"


def test_every_traced_call_has_a_footprint(lt, checked):
    _, called, ncalls = checked
    assert len(lt.cases()) == 45 and ncalls > 0
    missing = sorted(n for n in called if not fp.has_entry(n))
    assert not missing, f"no footprint entry for {missing}"
    # the suffixed forms the issue names are among the traced calls
    for n in ("l3u_norm_act_bwd_reduce_r1", "l3u_pw_bwd_tail_up", "l3u_outconv_bwd_ftl_dz",
              "l3u_outconv_bwd_loss4p_dz", "l3u_pw_bwd_tail_pair", "l3u_dw3_fwd_bf16"):
        assert n in called, f"{n} is no longer traced"


def test_table_names_are_bound_entry_points():
    unknown = sorted(n for n in list(fp.TABLE) + list(fp.SEGMENTS) if n not in nat._SIGS)
    assert not unknown, f"footprint entries for unknown entry points: {unknown}"
    for n, (names, _, _) in fp.TABLE.items():
        assert len(names.split()) + 1 == len(nat._SIGS[n]), f"{n}: argument count"
        for i, a in enumerate(names.split()):
            # *_ns are the long long batch strides, every other long long a count
            if a.endswith("_ns"):
                assert nat._SIGS[n][i] is nat.L, f"{n}: {a} is not a batch stride"
    for n, names in fp.SEGMENTS.items():
        assert len(names.split()) + 1 == len(nat._SIGS[n]), f"{n}: argument count"


def test_engine_plan_honours_the_table(checked):
    bad, _, ncalls = checked
    lines = [m for msgs in bad.values() for m in msgs]
    assert not lines, f"{len(lines)} violations in {ncalls} calls:\n" + "\n".join(lines[:40])


def test_table_conventions():
    """The conventions of include/l3u.h the issue lists, on hand-made calls."""
    # batch stride above C*S: N intervals (one half of a concat buffer); bf16 twin: E = 2
    args = (1 << 40, 2 * 3 * 100, (1 << 41), None, None, (1 << 42), 3 * 100, 2, 3, 4, 5, 5, 0)
    by = {o.arg: o for o in fp.footprints("l3u_dw3_fwd", args) if o.field is None}
    assert by[0].ivs == [(0, 1200), (2400, 3600)] and by[0].role == "r"
    assert by[5].ivs == [(0, 1200), (1200, 2400)] and by[5].role == "w"
    assert by[3].ivs == [] and by[3].ptr is None
    by = {o.arg: o for o in fp.footprints("l3u_dw3_fwd_bf16", args) if o.field is None}
    assert by[0].ivs == [(0, 600), (1200, 1800)] and by[2].ivs == [(0, 3 * 27 * 4)]
    # rank-1: a negative batch stride, one stored channel per sample
    r1 = (1 << 40, -100) + args[2:]
    by = {o.arg: o for o in fp.footprints("l3u_dw3_fwd", r1) if o.field is None}
    assert by[0].ivs == [(0, 400), (400, 800)]
    # a batch stride below one sample is refused
    with pytest.raises(ValueError):
        fp.footprints("l3u_dw3_fwd", (1 << 40, 100) + args[2:])
    # reduce items: fp32 rows, an fp64 strided column and an accumulating output
    rows = [[8, 3, 16, 1, 4, 0, 0, 0], [2, 2, 3, 6, 2, 10, 1, 1]]
    ops = fp.footprints("l3u_reduce_segments", (1 << 40, 1 << 41, 2, 1 << 42, 0), lambda p, n: rows)
    src = [o for o in ops if o.arg == 0][0]
    # fp32 elements 8..11, 24..27, 40..43; doubles 2, 5, 8, 11 (bytes 16, 40, 64, 88), joined
    assert src.ivs == [(16, 24), (32, 48), (64, 72), (88, 112), (160, 176)]
    dst = sorted((o.role, o.ivs) for o in ops if o.arg == 3)
    assert dst == [("rw", [(40, 48)]), ("w", [(0, 16)])]
    assert fp.footprints("l3u_ccl_label", (0,) * 10) is None


def test_fence_mask_paths_agree(monkeypatch):
    """tests/fenced.py _mask decides where the poison goes.  Its one-pass form (more than
    MASK_LOOP_MAX runs: the strided footprints of reduction items) and its run-by-run loop give the
    same mask, which is also a plain numpy restatement's: on random run lists (overlapping,
    touching, empty, inverted, leaving the block at either end) and on the merged ascending runs
    of a strided reduction item."""
    import torch

    import fenced
    dev = torch.device("cpu")
    rng = np.random.default_rng(11)

    def both(n, ivs):
        want = np.zeros(n, dtype=bool)
        for lo, hi in ivs:
            want[max(lo, 0):max(hi, 0)] = True
        monkeypatch.setattr(fenced, "MASK_LOOP_MAX", 10 ** 9)
        loop = fenced._mask(n, ivs, dev).numpy()
        monkeypatch.setattr(fenced, "MASK_LOOP_MAX", -1)
        fast = fenced._mask(n, ivs, dev).numpy()
        assert loop.dtype == fast.dtype == np.bool_ and loop.shape == fast.shape == (n,)
        assert np.array_equal(loop, want) and np.array_equal(fast, want)
        return want

    for _ in range(60):
        n = int(rng.integers(1, 4000))
        k = int(rng.integers(0, 600))
        lo = rng.integers(-60, n + 60, k)
        ivs = [(int(a), int(a + b)) for a, b in zip(lo, rng.integers(-6, 48, k))]
        both(n, ivs)
    assert both(16, [(12, 4), (2, 9)]).tolist() == [False] * 2 + [True] * 7 + [False] * 7
    assert not both(16, [(-9, -2), (16, 40), (5, 5)]).any() and both(8, [(-3, 99)]).all()
    # a strided fp64 column and fp32 rows, as the table hands them over (more runs than the
    # threshold the fence uses: the one-pass form is what a fenced reduction call gets)
    monkeypatch.undo()
    rows = [[3, 700, 2, 1400, 3, 0, 0, 1], [9000, 300, 8, 1, 4, 40, 0, 0]]
    ops = fp.footprints("l3u_reduce_segments", (1 << 40, 1 << 41, 2, 1 << 42, 0), lambda p, n: rows)
    ivs = [o for o in ops if o.arg == 0][0].ivs
    assert len(ivs) > fenced.MASK_LOOP_MAX
    m = both(46000, ivs)
    assert m.sum() == 700 * 3 * 8 + 300 * 4 * 4 and m[24] and not m[23] and not m[32]


def test_fenced_modules_name_only_known_entry_points():
    with open(os.path.join(ROOT, "tests", "test_fenced_ops_gpu.py")) as f:
        doc = f.read().split('"""')[1]
    listed = set(re.findall(r"l3u_\w+", doc.split("End guards only", 1)[1])) \
        if "End guards only" in doc else set()
    unknown = {}
    for mod in FENCED_SOURCES:
        with open(os.path.join(ROOT, "tests", mod + ".py")) as f:
            names = set(re.findall(r'"(l3u_\w+)"', f.read()))
        for n in sorted(names - nat._QUERIES):
            if n in nat._SIGS and not fp.has_entry(n) and n not in listed:
                unknown.setdefault(mod, []).append(n)
            # (a literal that is a prefix completed at run time, "l3u_outconv_bwd" + form, is
            # bound under its full names, which the traced and fenced calls check)
    assert not unknown, f"neither a footprint entry nor listed as end guards only: {unknown}"


def test_plan_check_sees_planted_faults(lt, monkeypatch):
    """The three properties on the smallest traced case with the table bent on purpose: a host
    query that promises one chunk fewer than the kernels lay out, and a producer whose partials
    are no longer counted as written."""
    case = {c.name: c for c in lt.cases()}["c8_10"]
    assert check_case(lt, case)[0] == []
    q = fp._q
    # the kernels write one chunk more than the engine was promised: the depthwise partials run
    # into the region laid out behind them
    monkeypatch.setattr(fp, "_q", lambda n, *a: q(n, *a) + (n == "l3u_dw3_nchunk"))
    bad = check_case(lt, case)[0]
    assert bad and all("l3u_dw3_bwd" in m for m in bad)
    assert any("overlap in bwd_arena" in m or "leaves bwd_arena" in m for m in bad)
    monkeypatch.setattr(fp, "_q", q)
    # nobody writes the block tail's partials: their readers and the final reduction are named
    names, fn, pairs = fp.TABLE["l3u_norm_act_bwd"]

    def unwritten(a, E):
        out = fn(a, E)
        out["part"] = ("r", out["part"][1])
        return out
    monkeypatch.setitem(fp.TABLE, "l3u_norm_act_bwd", (names, unwritten, pairs))
    bad = check_case(lt, case)[0]
    assert any("l3u_norm_act_bwd(" in m and "no earlier call wrote" in m for m in bad)
    assert any("l3u_reduce_segments(" in m and "no earlier call wrote" in m for m in bad)
