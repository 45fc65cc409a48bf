"""The engine's launch schedule as text, recorded on the CPU (no GPU needed).

With `_native.call` replaced by a recorder and `_native.stream` by a constant,
`UNetEngine.forward` / `backward` run on CPU tensors: they only allocate buffers, ask the
library's host queries and order C-ABI calls.  Every call and every engine allocation of two
consecutive steps is written as one text line, with pointers replaced by `buffer+byteoffset`, so
the text depends on the schedule alone.  tests/golden/launch_trace.json keeps one sha256 per case;
tests/test_launch_trace.py compares them, so a change of engine.py that alters any launch, argument,
buffer layout or reduction item shows up as a changed hash.  tests/test_footprints.py reads the
same steps' raw events and buffers (trace_raw) to hold every call against the footprint table.

usage: python tools/launch_trace.py            compare every case with the golden file
       python tools/launch_trace.py --dump CASE   print one case's text (diff two checkouts)
       python tools/launch_trace.py --list        case names
       python tools/launch_trace.py --write       regenerate the golden file
"""
import bisect
import ctypes
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-3d-unet-front_amd"))
import torch  # noqa: E402

from light_unet import _native as nat  # noqa: E402
from light_unet import engine as E  # noqa: E402
from light_unet.models.losses import family_descriptor  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.json")
SWITCHES = ("_FRONT", "_PAIR_PW", "_TAIL_FUSE", "_DWPW", "_PAIR_BWD", "_PAIR_TAIL_NARROW", "_RANK1",
            "_POOLFOLD", "_FRONT_R1", "_FUSE_ADAMW", "_SEG_SORT")
FTL = (0.7, 0.3, 0.75, 1e-6)
BIG, SMALL = (16, 32, 64, 128), (8, 16, 32, 64)


class Case:
    """One traced configuration.  loss: "dp" (dL/dp given, need_dx), "ftl" / "combined" / "dice"
    (formed in the out_conv backward); sums: the global sums are given instead of the forward's
    partials; opt: a stand-in optimizer (the fused AdamW reduction); train=False: eval forward
    only; off: engine switches set to False."""

    def __init__(self, name, enc, shape, bf16=False, dsep=True, grouped=True, loss="ftl",
                 sums=False, opt=False, train=True, off=()):
        self.name, self.enc, self.shape, self.bf16 = name, enc, shape, bf16
        self.dsep, self.grouped, self.loss, self.sums = dsep, grouped, loss, sums
        self.opt, self.train, self.off = opt, train, tuple(off)
        self.buf = None

    @property
    def family(self):
        if self.loss == "combined":
            return family_descriptor(0.8, *FTL, w_bce=0.2)
        if self.loss == "dice":
            return family_descriptor(w_dice=1.0, smooth_dice=1e-6)
        return None


def cases():
    out = [Case("c16_48", BIG, (1, 48, 48, 48), opt=True),
           Case("c16_48_bf16", BIG, (1, 48, 48, 48), opt=True, bf16=True),
           Case("c16_n2_32", BIG, (2, 32, 32, 32)),
           Case("c16_64", BIG, (1, 64, 64, 64)),
           Case("c8_16", SMALL, (1, 16, 16, 16)),
           Case("c8_12x20x16", SMALL, (1, 12, 20, 16)),
           Case("c8_10", SMALL, (1, 10, 10, 10)),
           Case("c8_10_bf16", SMALL, (1, 10, 10, 10), bf16=True),
           Case("c8_16_grouped", SMALL, (1, 16, 16, 16), dsep=False),
           Case("c8_16_dense", SMALL, (1, 16, 16, 16), dsep=False, grouped=False)]
    for tag, enc, shape in (("c16_48", BIG, (1, 48, 48, 48)), ("c8_16", SMALL, (1, 16, 16, 16))):
        out += [Case(tag + "_dp", enc, shape, loss="dp"),
                Case(tag + "_ftl_sums", enc, shape, sums=True),
                Case(tag + "_combined", enc, shape, loss="combined"),
                Case(tag + "_combined_sums", enc, shape, loss="combined", sums=True),
                Case(tag + "_dice", enc, shape, loss="dice")]
    out += [Case("c16_48_eval", BIG, (1, 48, 48, 48), train=False),
            Case("c8_12x20x16_eval", SMALL, (1, 12, 20, 16), train=False)]
    for sw in SWITCHES:
        out += [Case("c16_48_no" + sw, BIG, (1, 48, 48, 48), opt=True, off=(sw,)),
                Case("c16_n2_32_no" + sw, BIG, (2, 32, 32, 32), opt=True, off=(sw,))]
    out.append(Case("c16_48_dp_no_RANK1", BIG, (1, 48, 48, 48), loss="dp", off=("_RANK1",)))
    return out


class StandInAdamW:
    """What UNetEngine.backward reads of a FlatAdamW: g, p and fused_args()."""

    def __init__(self, p, g, counter):
        self.p, self.g, self.counter = p, g, counter
        self.m, self.v = torch.zeros_like(p), torch.zeros_like(p)
        self.lr = torch.zeros(1)
        self.step = torch.zeros(1, dtype=torch.int32)
        self.ticket = torch.zeros(32 * 33, dtype=torch.int32)

    def fused_args(self):
        return (self.g.data_ptr(), self.p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                self.lr.data_ptr(), 0.9, 0.999, 1e-8, 1e-5, self.step.data_ptr(), 1.0,
                self.ticket.data_ptr(), self.counter.data_ptr())

    def buffers(self):
        return {"opt_m": self.m, "opt_v": self.v, "opt_lr": self.lr, "opt_step": self.step,
                "opt_ticket": self.ticket}


def make_buffers(engine, case):
    """The CPU tensors of one case, by their fixed labels."""
    N, D, H, W = case.shape
    ncol = 3 if case.family is None else 4
    nparts = N * nat.query("l3u_outconv_nblocks", D * H * W)
    b = {"flat": torch.zeros(engine.numel), "gflat": torch.zeros(engine.numel),
         "x": torch.zeros(N, 1, D, H, W), "target": torch.zeros(N, 1, D, H, W),
         "counter": torch.zeros(1, dtype=torch.int32), "partials": torch.zeros(nparts * ncol),
         "sums": torch.zeros(ncol, dtype=torch.float64), "loss": torch.zeros(()),
         "dp": torch.zeros(N, 1, D, H, W)}
    case.nparts = nparts
    case.optim = StandInAdamW(b["flat"], b["gflat"], b["counter"]) if case.opt else None
    if case.optim is not None:
        b.update(case.optim.buffers())
    return b


def run_step(engine, case):
    """One forward (and backward) of `case` on its buffers, the way its caller drives the engine:
    TrainStep for the in-launch losses, the autograd function for a given dL/dp."""
    b = case.buf
    if not case.train:
        engine.forward(b["flat"], b["x"], training=False, save=False)
        return
    if case.loss == "dp":
        _, sv = engine.forward(b["flat"], b["x"], training=True, dropout_p=0.1,
                               counter=b["counter"], save=True)
        engine.backward(b["flat"], b["gflat"], sv, b["dp"], need_dx=True, opt=case.optim)
        return
    fam = case.family
    head = E.LossHead(b["target"], b["partials"], case.nparts, out=b["loss"], family=fam,
                      ftl=None if fam is not None else FTL)
    _, sv = engine.forward(b["flat"], b["x"], training=True, dropout_p=0.1, counter=b["counter"],
                           bump_counter=False, save=True, loss=head)
    if fam is not None:
        head.family = fam[:6] + (float(b["x"].numel()),) + fam[7:]
    if case.sums:
        head.sums = b["sums"]
    engine.backward(b["flat"], b["gflat"], sv, None, need_dx=False, loss=head, opt=case.optim)


class Recorder:
    """Events of the traced steps: ("alloc", tensor) and ("call", name, args)."""

    def __init__(self):
        self.events = []
        self.allocs = []

    def wrap(self, engine):
        """Stub the native calls and log the engine's allocations (as bench.StepRecorder.wrap
        does); returns the restore function."""
        orig_call, orig_stream = nat.call, nat.stream
        e_empty, e_f32 = engine._empty, engine._f32

        def logged(fn):
            def alloc(*a, **k):
                t = fn(*a, **k)
                self.allocs.append(t)
                self.events.append(("alloc", t))
                return t
            return alloc

        nat.call = lambda name, *args: self.events.append(("call", name, args))
        nat.stream = lambda: 0
        engine._empty, engine._f32 = logged(e_empty), logged(e_f32)

        def restore():
            nat.call, nat.stream = orig_call, orig_stream
            del engine._empty, engine._f32   # back to the class methods
        return restore


class Canon:
    """Arguments as text: numbers literally, pointers as label+byteoffset."""

    def __init__(self, labelled):
        self.table = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name)
                            for name, t in labelled.items())
        self.starts = [lo for lo, _, _ in self.table]

    def arg(self, a):
        if a is None:
            return "None"
        if isinstance(a, bool):
            return str(int(a))
        if isinstance(a, float):
            return repr(a)
        if isinstance(a, int):
            if a < 2 ** 32:
                return str(a)
            k = bisect.bisect_right(self.starts, a) - 1
            if k >= 0 and a < self.table[k][1]:
                return f"{self.table[k][2]}+{a - self.table[k][0]}"
            raise ValueError(f"argument {a:#x} is an address of no known buffer")
        if isinstance(a, ctypes._Pointer):
            s = a.contents
            return "{" + ", ".join(f"{f[0]}={self.arg(getattr(s, f[0]))}" for f in s._fields_) + "}"
        raise TypeError(f"argument of type {type(a).__name__}: {a!r}")

    def event(self, ev):
        if ev[0] == "alloc":
            return f"alloc {tuple(ev[1].shape)} {ev[1].dtype}"
        return f"{ev[1]}({', '.join(self.arg(a) for a in ev[2])})"


def trace_raw(case):
    """(events, labelled buffers, trailing text lines) of one case: the Recorder's raw events with
    their live pointer arguments, and every tensor those pointers fall in by its label (the
    case's buffers, the engine's allocations a0.., the arenas and the item table)."""
    saved = {sw: getattr(E, sw) for sw in case.off}
    for sw in case.off:
        setattr(E, sw, False)
    try:
        engine = E.UNetEngine(encoder_channels=case.enc, use_depthwise_separable=case.dsep,
                              use_grouped=case.grouped)
        if case.bf16:
            engine.set_act_dtype(torch.bfloat16)
        case.buf = make_buffers(engine, case)
        rec = Recorder()
        restore = rec.wrap(engine)
        try:
            for _ in range(2):   # the second step reuses the arenas planned by the first
                run_step(engine, case)
        finally:
            restore()
    finally:
        for sw, v in saved.items():
            setattr(E, sw, v)
    # every tensor of the case is still alive here (rec, case.buf, the engine), so no address
    # has been reused
    labelled = dict(case.buf)
    labelled.update({f"a{k}": t for k, t in enumerate(rec.allocs)})
    tail = []
    for key, t in engine._arenas.items():
        which = "fwd_arena" if key[0] == "f" else "bwd_arena"
        assert which not in labelled, "one shape per case"
        labelled[which] = t
        tail.append(f"{which} {t.numel()}")
    for key, items in engine._items.items():
        labelled["items"] = items
        tail += ["item " + " ".join(str(v) for v in row) for row in items.tolist()]
        tail.append(f"cover_once {engine._cover_once[key]}")
    tail.append(f"applied_update {engine.applied_update}")
    case.buf = case.optim = None
    return rec.events, labelled, tail


def trace(case):
    """(canonical text, number of calls, names called) of one case."""
    events, labelled, tail = trace_raw(case)
    canon = Canon(labelled)
    lines = [canon.event(ev) for ev in events] + tail
    names = [ev[1] for ev in events if ev[0] == "call"]
    return "\n".join(lines) + "\n", len(names), set(names)


def engine_entry_points():
    """Launch entry points that engine.py names in "l3u_..." string literals (not the host
    queries)."""
    with open(E.__file__) as f:
        names = set(re.findall(r'"(l3u_\w+)"', f.read()))
    return names - nat._QUERIES


def trace_all():
    """([{name, calls, sha256}], names called by any case with _bf16 stripped)."""
    rows, called = [], set()
    for case in cases():
        text, ncalls, names = trace(case)
        rows.append({"name": case.name, "calls": ncalls,
                     "sha256": hashlib.sha256(text.encode()).hexdigest()})
        called |= {n[:-5] if n[:-5] in nat.BF16_TWINS else n for n in names}
    return rows, called


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def main(argv):
    if "--list" in argv:
        print("\n".join(c.name for c in cases()))
        return 0
    if "--dump" in argv:
        want = argv[argv.index("--dump") + 1]
        case = next(c for c in cases() if c.name == want)
        sys.stdout.write(trace(case)[0])
        return 0
    rows, called = trace_all()
    missing = sorted(engine_entry_points() - called)
    if missing:
        print("entry points no case reaches:", ", ".join(missing))
    if "--write" in argv:
        with open(GOLDEN, "w") as f:
            json.dump({"cases": rows}, f, indent=1)
            f.write("\n")
        print(f"wrote {len(rows)} cases to {GOLDEN}")
        return 1 if missing else 0
    gold = {r["name"]: r for r in load_golden()}
    bad = [r["name"] for r in rows if gold.get(r["name"]) != r]
    bad += sorted(set(gold) - {r["name"] for r in rows})
    print(f"{len(rows)} cases, {len(bad)} differ from the golden file" +
          (": " + ", ".join(bad) if bad else ""))
    return 1 if bad or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
