"""Benchmark: Lightweight3DUNet training throughput on MI355X (BASELINE.json `metric`).

Workload (BASELINE.json configs[1]): 16->32->64->128 U-Net, 48^3 patches,
batch 4 per GPU, fp32, dropout 0.1, FocalTversky(0.7, 0.3, 0.75), AdamW(lr 1e-4, wd 1e-5).
A step = forward + loss + backward + optimizer (trainer.py:222-232) over one synthetic batch,
replayed from a hipGraph; inputs are generated on the host before timing and are resident in HBM
(a pool of 8 distinct batches, each copied device-to-device into the graph's input buffer inside
the timed step: one copy of image + target).  N > 1: one process per GPU (torch.distributed.run), exact global-batch FocalTversky
(3-float all-reduce) + one flat-gradient RCCL all-reduce per step; per-GPU batch fixed (weak
scaling); time = max over ranks.

A plain run (`bench.py --gpus N --steps K --warmup W`) sets up, warms up, times the K steps and
prints the result line (metric, value, unit, ms_per_step, ...).  `--dump-outputs DIR` also
writes what the last timed step gave its caller (loss, updated flat parameters, flat gradient)
as DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.

With `--full` also reported: eval forward ms/patch (bs 1 and 4), config 5 (32->256, 64^3,
step-based mixed domains) data-parallel over the job's GPUs, the grouped-conv variant on one GPU,
the config-4 whole-volume sliding-window
inference of a 256^3 synthetic PET volume (seconds, ms/window; light_unet.utils), the roofline of
the dominant kernel measured with HIP events around back-to-back replays of its C-ABI call, and
the CPU baseline (the torch-CPU oracle restatement of the same network on this host's cores,
rank 0 only, bounded sample).  The `--no-*` options drop single legs of a `--full` run.  The
headline step is the same with and without `--full`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "light-3d-unet-front_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
METRIC = "train patches/sec (48³, bs=4/GPU) at 1/2/4/8 MI355X + fwd ms/patch"


def parse():
    ap = argparse.ArgumentParser()
    # default: WORLD_SIZE under a launcher (torchrun --nproc-per-node N bench.py), else 1
    ap.add_argument("--gpus", type=int, default=None)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--enc", type=str, default="16,32,64,128")
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"],
                    help="activation storage of the headline step (bf16: BASELINE config 3)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=40)   # ~10-30 s of host work
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-bf16", action="store_true", help="skip the bf16 (config 3) step timing")
    ap.add_argument("--no-dropin", action="store_true", help="skip the drop-in autograd step timing")
    ap.add_argument("--no-data", action="store_true",
                    help="skip the data-path timings (lesion post-processing, training patches)")
    ap.add_argument("--ftl-mode", default="exact", choices=["exact", "local"])
    ap.add_argument("--no-sliding", action="store_true", help="skip the config-4 inference timing")
    ap.add_argument("--no-config5", action="store_true", help="skip the config-5 (32->256, 64^3) timing")
    ap.add_argument("--no-exchange", action="store_true",
                    help="skip the one-GPU RCCL exchange probe (tools/rccl_probe.py)")
    ap.add_argument("--no-grouped", action="store_true",
                    help="skip the use_depthwise_separable=False (grouped) model timing")
    # multi-rank rehearsal on a one-GPU box: every rank on cuda:0, collectives over gloo
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--one-device", action="store_true")
    ap.add_argument("--dump-calls", default=None,
                    help="(with --full) write the recorded step's C-ABI calls (name, family, label, algorithmic "
                         "bytes) in launch order to this JSON file (tools/instep.py aligns them "
                         "with a rocprofv3 kernel trace of the graph-replayed step)")
    ap.add_argument("--full", action="store_true",
                    help="also run every side leg (eval forward, sliding window, config 5, grouped, "
                         "bf16, drop-in, data path, exchange probe, rooflines, CPU baseline); a "
                         "plain run times the headline step only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last one gave its caller (loss, "
                         "params, grads) as DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_calls and not args.full:
        ap.error("--dump-calls records the roofline leg's step: add --full")
    if args.gpus is None:
        args.gpus = int(os.environ.get("WORLD_SIZE", "1"))
    return args


def synthetic_pool(n_pool, bs, size, rank, device):
    """n_pool batches resident in HBM, each image and target side by side in ONE buffer
    [2, bs, 1, D, H, W] so that staging a batch into the graph's inputs is one copy."""
    pool = []
    for i in range(n_pool):
        rng = np.random.default_rng(42 + 1000 * rank + i)
        x = rng.random((bs, 1, size, size, size), dtype=np.float32)
        t = (rng.random((bs, 1, size, size, size)) > 0.97).astype(np.float32)
        pool.append(torch.from_numpy(np.stack([x, t])).to(device))
    return pool


DUMP_BUDGET = 64 * 2 ** 20   # bytes, over all arrays of one --dump-outputs


def dump_outputs(dirname, arrays):
    """Write {name: device tensor} as dirname/<name>.npy (float32).  An array is written whole
    while it fits an equal share of DUMP_BUDGET, a larger one as a fixed sample (seed 0) of its
    flattened elements: the same indices in every run."""
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_BUDGET // (4 * len(arrays))   # elements per array
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.size > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), a)


def dw_bytes(N, C, S, e=4, acc=0):
    """Algorithmic HBM bytes of one depthwise backward (data + weight gradient):
    read dZ + write dX (fp32 gradients) + read X (e = 4 fp32 / 2 bf16 activations) + 27 weights,
    + read dX when the call accumulates into it (acc)."""
    return 4 * ((2 + acc) * N * C * S) + e * N * C * S + 4 * 27 * C


def pmc_traffic(N, C, size, acc=0):
    """Memory-side bytes per call of the dominant kernel from the committed rocprofv3 PMC passes
    (tools/pmc.sh -> profiles/*_pmc_dw3_bwd.json) taken at this exact shape and mode, preferring
    the record made on this product tree.  (bytes, source, tree_matches)."""
    def ok(rec):
        call = rec.get("call", "")
        return f"[{N},{C},{size}^3]" in call and f"accumulate={acc}" in call
    rec, fn, same = _pick_record("*_pmc_dw3_bwd.json", ok)
    if rec is None or not ok(rec):
        return None, None, False
    return rec["traffic_bytes"], os.path.relpath(fn, ROOT) + " (FETCH_SIZE x2 + WRITE_SIZE)", same


class KernelTimer:
    """Captures the arguments of the C-ABI calls that make up the dominant operation (at their
    real shapes and buffers) during one eager step, then re-issues exactly those calls
    back-to-back between two HIP events on one stream: the average is the kernels' own
    duration, free of event/launch gaps."""

    def __init__(self, names, match):
        self.names, self.match, self.args = names, match, {}

    def wrap(self, nat):
        orig = nat.call

        def call(name, *args):
            if name in self.names and self.match(args) and name not in self.args:
                self.args[name] = args
            orig(name, *args)
        nat.call = call
        return orig

    def mean_ms(self, nat_call, reps=50):
        """Mean over `reps` back-to-back calls between two HIP events on the launch stream (one
        continuous batch: syncs between shorter batches let the clocks drop and read ~15% slow)."""
        if set(self.args) != set(self.names):
            return None
        s = torch.cuda.current_stream()

        def issue():
            for name in self.names:
                nat_call(name, *self.args[name][:-1], s.cuda_stream)
        for _ in range(3):
            issue()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps):
            issue()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps


class StepRecorder:
    """Records every C-ABI call (name, arguments: real shapes and buffers) of one eager training
    step; `time_calls` then re-issues selected calls back-to-back between two HIP events on the
    launch stream, giving each call's own average duration (warm caches: the call's inputs were
    just touched, so the MALL may serve part of them; the rocprof in-step figures are in
    profiles/)."""

    def __init__(self):
        self.calls = []
        self.keep = []

    def wrap(self, nat, engine):
        """Record nat.call; every activation / workspace tensor the engine allocates during the
        recorded step is kept alive here, so that re-issued calls touch only live buffers
        (host-side argument structs are kept alive by their pointer objects, _native.norm_src_ptr).
        Returns the restore function."""
        orig = nat.call
        e_empty, e_f32 = engine._empty, engine._f32

        def call(name, *args):
            self.calls.append((name, args))
            orig(name, *args)

        def empty(*a, **k):
            t = e_empty(*a, **k)
            self.keep.append(t)
            return t

        def f32(*a, **k):
            t = e_f32(*a, **k)
            self.keep.append(t)
            return t
        nat.call = call
        engine._empty, engine._f32 = empty, f32

        def restore():
            nat.call = orig
            del engine._empty, engine._f32   # back to the class methods
        self.orig = orig
        return restore

    @staticmethod
    def time_calls(nat_call, calls, reps=20):
        s = torch.cuda.current_stream()
        out = []
        for name, args in calls:
            a = args[:-1] + (s.cuda_stream,)
            for _ in range(3):
                nat_call(name, *a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                nat_call(name, *a)
            e1.record(s)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / reps)
        return out


def _e(name):
    return 2 if name.endswith("_bf16") else 4


# reduction items of the recorded step by device pointer (engine._items), for the byte model of
# the weight-gradient reduction launch
SEG_ITEMS = {}


def seg_items_from(engine):
    SEG_ITEMS.clear()
    for t in engine._items.values():
        SEG_ITEMS[t.data_ptr()] = t.cpu().tolist()


def call_bytes(name, a):
    """Algorithmic HBM bytes of one C-ABI call from its arguments (activations e = 4
    (fp32) or 2 (the _bf16 twins), gradients fp32), with a shape label; None when the call is not
    in the depthwise, GEMM or reduction families."""
    e, base = _e(name), name[:-5] if name.endswith("_bf16") else name
    if base in ("l3u_reduce_segments", "l3u_reduce_segments_adamw") and a[1] in SEG_ITEMS:
        # (src, items, nitems, ...): every partial read once (fp32, or fp64 for the IN affine
        # partials), the 64-byte item table, and per output the gradient write plus (adamw) the
        # parameter and both moments read and written
        rows = SEG_ITEMS[a[1]]
        part = sum(r[1] * r[4] * (8 if r[7] else 4) for r in rows)
        nout = sum(r[4] for r in rows)
        per = 28 if base.endswith("adamw") else 4
        return ("reduce", f"{base[4:]} {len(rows)} items, {part / 1e6:.1f} MB partials",
                part + 64 * len(rows) + per * nout + 4 * sum(r[4] for r in rows if r[6]))
    if base == "l3u_dw3_fwd":     # (x, xns, w, rec, src, y, yns, N, C, D, H, W)
        N, C, D, H, W = a[7:12]
        S = D * H * W
        return "dw", f"fwd [{N},{C},{D}x{H}x{W}]", e * 2 * N * C * S + 108 * C
    if base == "l3u_dw3_bwd":     # (dz, dzns, x, xns, w, rec, dx, dxns, acc, dwp, inp, N, C, D, H, W)
        N, C, D, H, W = a[11:16]
        S = D * H * W
        acc = a[8]
        ca = 1 if a[3] < 0 else C   # a rank-1 input (negative stride) reads one channel
        return ("dw", f"bwd{'+IN' if a[5] else ''}{'+acc' if acc else ''}{' (rank-1 A)' if a[3] < 0 else ''} "
                      f"[{N},{C},{D}x{H}x{W}]", 4 * N * C * S * (2 + acc) + e * N * ca * S + 108 * C)
    if base == "l3u_pw_fwd":      # (x, xns, w, trans, bias, y, yns, acc, part, N, K, J, S)
        N, K, J, S = a[9:13]
        if a[3]:                  # W^T dy of a backward (fp32 operands)
            e = 4
        return "gemm", f"pw_fwd{'T' if a[3] else ''} {K}->{J} [{N},{S}]", e * N * S * (K + J * (1 + a[7]))
    if base == "l3u_pw_fwd2":     # (x, xns, wr, r, rns, so, z1, z1ns, w1, y1, y1ns, s1, N, K, J, S)
        N, K, J, S = a[12:16]
        return "gemm", f"pw_fwd2 2x{K}->{J} [{N},{S}]", e * N * S * 2 * (K + J)
    if base == "l3u_pw_bwd":      # (dy, dyns, y, yns, rec, ip, np, x, xns, w, dx, dxns, acc, part, N, J, K, S)
        N, J, K, S = a[14:18]
        pro = a[2] is not None
        jy = 1 if (pro and a[3] < 0) else J   # rank-1 y
        return ("gemm", f"pw_bwd {J}->{K}{'+IN' if pro else ''} [{N},{S}]",
                N * S * (4 * J + (e * jy if pro else 0) + e * K + 4 * K * (1 + a[12])))
    if base == "l3u_pw_bwd_tail":  # (dout, dns, out, ons, yr, yns, rec, pn, ntp, sel, x, xns, w, dx, dxns, acc, part, N, J, K, S)
        N, J, K, S = a[17:21]
        jr = 1 if a[5] < 0 else J   # rank-1 yr
        return ("gemm", f"pw_bwd_tail{a[9]} {J}->{K} [{N},{S}]",
                N * S * (4 * J + e * (J + jr) + e * K + 4 * K * (1 + a[15])))
    if base == "l3u_pw_bwd_tail_r1":  # (dz, dzns, dscale, out, ons, yr, yns, rec, pn, ntp, sel, x, xns, w, dx, dxns, acc, part, N, J, K, S)
        N, J, K, S = a[18:22]           # rank-1 dout: one fp32 channel
        jr = 1 if a[6] < 0 else J
        return ("gemm", f"pw_bwd_tail{a[10]} (rank-1 dout) {J}->{K} [{N},{S}]",
                N * S * (4 + e * (J + jr) + e * K + 4 * K * (1 + a[16])))
    if base == "l3u_pw_bwd_tail_up":  # (dskip, dskns, dpool, dpns, idx, out, ons, yr, yns, rec, pn, ntp, sel, x, xns, w, dx, dxns, acc, part, N, J, K, D, H, W)
        N, J, K, D, H, W = a[20:26]     # dout = skip gradient + unpooled dpool (+ argmax bytes)
        S = D * H * W
        jr = 1 if a[8] < 0 else J
        return ("gemm", f"pw_bwd_tail{a[12]} (+maxpool bwd) {J}->{K}{' (rank-1 r)' if a[8] < 0 else ''} [{N},{S}]",
                N * S * (4 * J + 4 * J / 8 + J / 8 + e * (J + jr) + e * K + 4 * K * (1 + a[18])))
    if base == "l3u_pw_bwd2":     # two plain pw_bwd problems: (dy, dyns, x, xns, w, dx, dxns, acc, part, K) x 2, N, J, S
        N, J, S = a[20:23]
        Ka, Kb = a[9], a[19]
        return ("gemm", f"pw_bwd2 {J}->{Ka} + {J}->{Kb} [{N},{S}]",
                N * S * sum(4 * J + e * K + 4 * K * (1 + acc) for K, acc in ((Ka, a[7]), (Kb, a[17]))))
    if base == "l3u_pw_bwd_tail_pair":  # (dout, dns, dscale, dpool, dpns, idx, Hf, Wf, out, ons, pn, ntp, (yr, yns, rec, x, xns, w, dx, dxns, acc, part, K, sel) x 2, N, J, S)
        N, J, S = a[36:39]
        dj = 1 if a[2] is not None else J                      # rank-1 dout
        pool = (4 * J / 8 + J / 8) if a[3] is not None else 0  # unpooled dpool + argmax bytes
        form = " (rank-1 dout)" if a[2] is not None else (" (+maxpool bwd)" if a[3] is not None else "")
        tot = 0
        for o in (12, 24):   # each problem reads the tail operands (dout, out) itself
            K, acc = a[o + 10], a[o + 8]
            tot += N * S * (4 * dj + pool + e * 2 * J + e * K + 4 * K * (1 + acc))
        return ("gemm", f"pw_bwd_tail pair{form} {J}->{a[22]} + {J}->{a[34]} [{N},{S}]", tot)
    if base == "l3u_pw_bwd_weight":  # (dy, dyns, x, xns, part, N, J, K, S)
        N, J, K, S = a[5:9]
        return "gemm", f"pw_bwd_weight {J}x{K} [{N},{S}]", N * S * (4 * J + e * K)
    if base == "l3u_convt_fwd":   # (x, xns, w, b, y, yns, N, ci, co, d, h, w)
        N, ci, co, d, h, w = a[6:12]
        Si = d * h * w
        return "gemm", f"convt_fwd {ci}->{co} [{N},{d}x{h}x{w}]", e * N * Si * (ci + 8 * co)
    if base in ("l3u_convt_bwd", "l3u_convt_bwd_fused"):  # (dcat, dns, prev, pns, w, dprev, dpns, pw, pb, N, ci, co, d, h, w)
        N, ci, co, d, h, w = a[9:15]
        Si = d * h * w
        return "gemm", f"convt_bwd {ci}<-{co} [{N},{d}x{h}x{w}]", N * Si * (4 * 8 * co + e * ci + 4 * ci)
    if base == "l3u_dwpw_fwd":    # (x, xns, wdw, rec, src, wpw, y, yns, ys, wsc, r, rns, rs, z, zns, N, K, J, D, H, W)
        N, K, J, D, H, W = a[15:21]
        S = D * H * W
        sc = a[9] is not None
        kin = 1 if a[1] < 0 else K   # a rank-1 input reads one channel
        return ("dw", f"dwsep fwd (dw + pw{' + shortcut' if sc else ''}){' (rank-1 input)' if a[1] < 0 else ''} "
                      f"[{N},{K}->{J},{D}x{H}x{W}]",
                e * N * S * (kin + J * (1 + sc) + (K if a[13] is not None else 0)) + 4 * K * (27 + J * (1 + sc)))
    if base == "l3u_front_fwd":   # (x, xns, wdw, wpw, wsc, z1, y1, r, s1, so, xc, N, cout, d, h, w)
        N, co, d, h, w = a[11:16]
        S = d * h * w
        nw = (co if a[6] else 0) + (co if a[7] else 0)   # y1 / r not written when rank-1
        return ("dw", f"front (1ch dw{' + 2 rank-1 pw' if nw else ''}) [{N},1->{co},{d}x{h}x{w}]",
                4 * N * S + e * N * S * (1 + nw + (1 if a[10] else 0)))
    # ---- the InstanceNorm / block-tail family (norm.hip) and the out_conv + loss launches
    if base == "l3u_norm_act_fwd":   # (y2, y2ns, rec2, src2, r, rns, rec_r, src_r, sc, out, ons, N, C, S)
        N, C, S = a[11:14]
        cr = 1 if a[5] < 0 else C     # rank-1 residual: one stored channel
        return "norm", f"block tail fwd [{N},{C},{S}]", e * N * S * (2 * C + cr)
    if base == "l3u_norm_act_pool_fwd":  # (..., out, ons, pooled, pns, idx, N, C, D, H, W)
        N, C, D, H, W = a[14:19]
        S = D * H * W
        cr = 1 if a[5] < 0 else C
        return ("norm", f"block tail fwd + maxpool [{N},{C},{D}x{H}x{W}]",
                e * N * S * (2 * C + cr) + N * C * (S // 8) * (e + 1))
    if base == "l3u_norm_act_bwd_reduce":  # (dout, dns, out, ons, y2, y2ns, rec2, r, rns, rec_r, part, N, C, S)
        N, C, S = a[11:14]
        cr = 1 if a[8] < 0 else C
        return "norm", f"block tail bwd reduce [{N},{C},{S}]", N * S * (4 * C + e * (2 * C + cr))
    if base == "l3u_norm_act_bwd_reduce_r1":  # (dz, dzns, dscale, out, ons, y2, y2ns, rec2, r, rns, rec_r, part, N, C, S)
        N, C, S = a[12:15]
        cr = 1 if a[9] < 0 else C
        return "norm", f"block tail bwd reduce (rank-1 dout) [{N},{C},{S}]", N * S * (4 + e * (2 * C + cr))
    if base == "l3u_norm_act_bwd_reduce_up":  # (dout, dns, dpool, dpns, idx, out, ons, y2, y2ns, rec2, r, rns, rec_r, part, N, C, D, H, W)
        N, C, D, H, W = a[14:19]
        S = D * H * W
        cr = 1 if a[11] < 0 else C
        return ("norm", f"block tail bwd reduce (+maxpool bwd) [{N},{C},{D}x{H}x{W}]",
                N * S * (4 * C + e * (2 * C + cr)) + N * C * (S // 8) * 5)
    if base in ("l3u_norm_act_bwd_apply", "l3u_norm_act_bwd"):  # (dout, dns, out, ons, y2, y2ns, rec2, r, rns, rec_r, part, dy2, dy2ns, dr, drns, N, C, S)
        N, C, S = a[15:18]
        return ("norm", f"block tail bwd{' (one launch)' if base == 'l3u_norm_act_bwd' else ' apply'} [{N},{C},{S}]",
                N * S * C * (4 + 3 * e + 8))
    if base == "l3u_norm_act_bwd_up":  # (dout, dns, dpool, dpns, idx, out, ons, y2, y2ns, rec2, r, rns, rec_r, part, dy2, dy2ns, dr, drns, N, C, D, H, W)
        N, C, D, H, W = a[18:23]
        S = D * H * W
        return ("norm", f"block tail bwd (one launch, +maxpool bwd) [{N},{C},{D}x{H}x{W}]",
                N * S * C * (4 + 3 * e + 8) + N * C * (S // 8) * 5)
    if base == "l3u_in_bwd_apply":   # (dy, dyns, y, yns, rec, ip, np, dx, dxns, N, C, S)
        N, C, S = a[9:12]
        return "norm", f"IN bwd apply [{N},{C},{S}]", N * C * S * (8 + e)
    if base == "l3u_maxpool2_fwd":   # (x, xns, y, yns, idx, N, C, D, H, W)
        N, C, D, H, W = a[5:10]
        S = D * H * W
        return "norm", f"maxpool fwd [{N},{C},{D}x{H}x{W}]", N * C * (e * S + (S // 8) * (e + 1))
    if base == "l3u_maxpool2_bwd":   # (dpool, dpns, idx, dskip, dskns, dlev, dlevns, N, C, D, H, W)
        N, C, D, H, W = a[7:12]
        S = D * H * W
        return "norm", f"maxpool bwd [{N},{C},{D}x{H}x{W}]", N * C * (8 * S + (S // 8) * 5)
    if base == "l3u_outconv_fwd":    # (h, hns, w, b, p, t, part, N, C, S)
        N, C, S = a[7:10]
        return "io", f"out_conv + sigmoid{' + FTL sums' if a[5] else ''} [{N},{C}->1,{S}]", \
            N * S * (e * C + 4 + (4 if a[5] else 0))
    if base in ("l3u_outconv_bwd", "l3u_outconv_bwd_dz", "l3u_outconv_bwd_ftl", "l3u_outconv_bwd_ftl_dz"):
        N, C, S = a[16:19]          # (dp | p, p | t, t | fpart, ..., h(9), hns, w, dh, dhns, part, loss, N, C, S)
        ftl = "ftl" in base or a[0] is None
        dz = base.endswith("_dz")
        rd = 4 * 2 if ftl else 4 * (2 if a[2] is None else 3)   # p, t (and dp)
        return ("io", f"out_conv + sigmoid{' + FTL' if ftl else ''} bwd{' (rank-1 dz)' if dz else ''} [{N},{C}->1,{S}]",
                N * S * (rd + e * C + (4 if dz else 4 * C)))
    return None


def family_rooflines(nat_call, calls):
    """Per-launch and aggregate achieved bandwidth of the depthwise and GEMM families of one
    training step (every call of the family, timed one by one)."""
    sel = []
    for name, args in calls:
        r = call_bytes(name, args)
        if r is not None and r[0] != "reduce":   # (re-running it would apply AdamW again)
            sel.append((name, args, r))
    ms = StepRecorder.time_calls(nat_call, [(n, a) for n, a, _ in sel])
    fam = {"dw": [], "gemm": [], "norm": [], "io": []}
    for (name, _, (f, label, b)), t in zip(sel, ms):
        fam[f].append({"call": label, "us": round(1000 * t, 2), "bytes": int(b),
                       "achieved": round(b / (t * 1e-3) / 1e9, 1),
                       "frac": round(b / (t * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
    out = {}
    for f, rows in fam.items():
        tb = sum(r["bytes"] for r in rows)
        tt = sum(r["us"] for r in rows) * 1e-6
        out[f] = {"launches": len(rows), "bytes": tb, "us": round(tt * 1e6, 1),
                  "achieved": round(tb / tt / 1e9, 1) if tt else None,
                  "frac": round(tb / tt / 1e9 / HBM_PEAK_GBS, 4) if tt else None, "calls": rows}
    return out


def _tree():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from treehash import product_tree
    return product_tree()


def _pick_record(pattern, ok=None):
    """The committed evidence record (profiles/<pattern>) that describes THIS product tree: the
    newest whose "tree" hash (tools/treehash.py, stored when the record was made) equals the
    running tree's; failing that the newest one `ok(rec)` accepts (e.g. the same launch count),
    flagged tree_matches = False.  (rec, path, tree_matches) or (None, None, False)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    recs = []
    for fn in files:
        with open(fn) as f:
            recs.append((json.load(f), fn))
    cur = _tree()
    for rec, fn in reversed(recs):
        if rec.get("tree") == cur:
            return rec, fn, True
    for rec, fn in reversed(recs):
        if ok is None or ok(rec):
            return rec, fn, False
    return None, None, False


def instep_evidence(workload, launches):
    """In-step family rooflines from the committed tools/instep.py record of this workload made on
    this product tree (a rocprofv3 kernel trace of the graph-replayed step aligned with its C-ABI
    calls: profiles/*_instep_<workload>.json); per family: launches, bytes, in-step us, achieved
    GB/s, fraction of 8 TB/s.  `matches_this_step`: the record's tree hash is this tree's and it
    has this step's launch count."""
    rec, fn, same_tree = _pick_record(
        f"*_instep_{workload}.json",
        (lambda r: r.get("calls") == launches) if launches is not None else None)
    if rec is None:
        return None
    ncalls = rec["dw"]["launches"] + rec["gemm"]["launches"]
    out = {"source": os.path.relpath(fn, ROOT), "commit": rec.get("commit"), "tree": rec.get("tree"),
           "tree_matches": same_tree,
           "step_kernel_us": rec["step_kernel_us"], "launches": rec["launches"],
           "under_10us": rec.get("under_10us")}
    for fam in ("dw", "gemm", "reduce", "norm", "io"):
        if fam in rec:
            out[fam] = {k: rec[fam][k] for k in ("launches", "bytes", "us", "achieved", "frac")}
    if "coverage" in rec:
        out["coverage"] = rec["coverage"]
    if "reduce" in rec and rec["reduce"]["calls"]:
        out["reduce"]["call"] = rec["reduce"]["calls"][0]["call"]
    out["dominant"] = max(rec["dw"]["calls"] + rec["gemm"]["calls"], key=lambda r: r["us"])
    out["family_calls"] = ncalls
    out["matches_this_step"] = (same_tree and (launches is None or rec.get("calls") == launches))
    return out


def step_traffic_evidence(workload, ms_per_step):
    """Whole-step HBM traffic of the eager step from the committed PMC record of this workload
    made on this product tree (tools/pmc_step.sh -> profiles/*_pmc_step_<workload>.json:
    FETCH_SIZE x 2 + WRITE_SIZE per launch, separate passes) and the average rate it implies at
    this step time."""
    rec, fn, same_tree = _pick_record(f"*_pmc_step_{workload}.json")
    if rec is None:
        return None
    b = rec["step_traffic_bytes"]
    out = {"source": os.path.relpath(fn, ROOT), "commit": rec.get("commit"), "tree": rec.get("tree"),
           "tree_matches": same_tree, "bytes": b, "launches": rec.get("launches")}
    if ms_per_step:
        out["avg_tb_s"] = round(b / (ms_per_step * 1e-3) / 1e12, 3)
        out["frac_of_8tb_s"] = round(out["avg_tb_s"] / 8.0, 4)
    return out


def gemm_mfma_evidence(top=5):
    """MFMA-busy fractions of the step's GEMM launches from the committed rocprofv3 passes
    (tools/pmc_step.sh + tools/pmc_gemm.sh -> tools/pmc_launch_json.py -> profiles/*_pmc_step.json),
    the record made on this product tree first."""
    def ok(rec):
        return any("mfma_util" in i and i.get("mfma_busy_cycles", 0) > 0 for i in rec.get("items", []))
    rec, src, same = _pick_record("r*_pmc_step.json", ok)
    if rec is None or not ok(rec):
        return None
    items = [i for i in rec["items"] if "mfma_util" in i and i.get("mfma_busy_cycles", 0) > 0]
    items.sort(key=lambda i: -i["pmc_dur_us"])
    return {"source": os.path.relpath(src, ROOT), "tree_matches": same,
            "definition": "SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 * 1024 SIMDs)",
            "ceiling_note": "fp32 MFMA at the HBM roofline: 5.5 flop/B x 8 TB/s = 44 TFLOP/s = 0.28 of "
                            "the 157 TFLOP/s fp32 matrix peak",
            "top": [{"kernel": i["kernel"], "pmc_dur_us": i["pmc_dur_us"],
                     "mfma_util": round(i["mfma_util"], 4), "traffic": int(i["traffic"])}
                    for i in items[:top]]}


def dw_bwd_cache_exceeding(device, N=8, C=32, L=48, reps=30):
    """The dominant call's kernel (single-pass depthwise backward, mode 0) at a batch whose
    working set (dZ + X + dX = 340 MB at [8, 32, 48^3]) exceeds the 256 MB MALL, as SURVEY §8d
    asks: HIP events around back-to-back launches on the launch stream."""
    from light_unet import _native as nat
    S = L ** 3
    g = torch.Generator(device=device).manual_seed(3)
    dz = torch.randn(N, C, S, device=device, generator=g)
    x = torch.randn(N, C, S, device=device, generator=g)
    dx = torch.empty(N, C, S, device=device)
    w = torch.randn(C, 27, device=device, generator=g)
    nch = nat.query("l3u_dw3_nchunk", N, C, L, L, L)
    part = torch.empty(C * N * nch * 27, device=device)
    st = torch.cuda.current_stream()

    def call():
        nat.call("l3u_dw3_bwd", dz.data_ptr(), C * S, x.data_ptr(), C * S, w.data_ptr(), None,
                 dx.data_ptr(), C * S, 0, part.data_ptr(), None, N, C, L, L, L, st.cuda_stream)
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call()
    e1.record(st)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    b = dw_bytes(N, C, S)
    return {"call": f"l3u_dw3_bwd [{N},{C},{L}^3]", "working_set_MB": round(3 * 4 * N * C * S / 1e6, 1),
            "algorithmic_bytes": b, "avg_launch_ms": round(ms, 5),
            "achieved": round(b / (ms * 1e-3) / 1e9, 1), "frac": round(b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def cpu_baseline(args, enc):
    """The oracle (torch-CPU restatement of the same network, fp32) on the host cores."""
    from oracle import unet_oracle as U
    from light_unet.engine import param_layout
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS", "16")))))
    g = torch.Generator().manual_seed(0)
    sd = {}
    for name, shape in param_layout(enc):
        sd[name] = (torch.randn(shape, generator=g) * 0.1).requires_grad_(True)
    opt = torch.optim.AdamW(list(sd.values()), lr=1e-4, weight_decay=1e-5)
    rng = np.random.default_rng(42)
    bs, size = args.batch, args.size
    x = torch.from_numpy(rng.random((bs, 1, size, size, size), dtype=np.float32))
    t = torch.from_numpy((rng.random((bs, 1, size, size, size)) > 0.97).astype(np.float32))

    # Dropout3d(p) after norm1 of every ResidualBlock, as the GPU step runs it (unet3d.py:84-88):
    # one Bernoulli(1-p) keep flag per (sample, channel), fresh every step
    drop_p = args.dropout
    blocks = [k[:-len("norm1.weight")] for k in sd if k.endswith("norm1.weight")]

    def step():
        masks = {b: (torch.rand(bs, sd[b + "norm1.weight"].shape[0], generator=g) >= drop_p).float()
                 for b in blocks} if drop_p > 0 else None
        out = U.unet_forward(sd, x, drop_masks=masks, drop_p=drop_p)
        loss = U.focal_tversky(out, t)
        opt.zero_grad()
        loss.backward()
        opt.step()

    warm = 3
    for _ in range(warm):
        step()
    t0 = time.perf_counter()
    for _ in range(args.cpu_steps):
        step()
    dt = time.perf_counter() - t0
    return {"value": round(args.cpu_steps * bs / dt, 3), "unit": "patches/s",
            "cores": torch.get_num_threads(), "kind": "port", "cpu_model": cpu_model(),
            "sample": f"{args.cpu_steps} train steps (fwd+FocalTversky+bwd+AdamW, Dropout3d "
                      f"p={drop_p}) of bs={bs} {size}^3 fp32 after {warm} warm-ups, "
                      f"oracle/unet_oracle.py (aten CPU)",
            "ms_per_step": round(1000 * dt / args.cpu_steps, 1)}


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def fwd_ms_per_patch(model, bs, size, device, iters=20):
    x = torch.rand(bs, 1, size, size, size, device=device)
    model.eval()
    with torch.no_grad():
        for _ in range(3):
            model(x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model(x)
        torch.cuda.current_stream().wait_stream(s)
        with torch.cuda.graph(g):
            model(x)
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            g.replay()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    model.train()
    return 1000 * dt / iters / bs


def synthetic_pet(size=256, seed=42):
    """background U[0,0.05), central ellipsoid body U[0.1,0.4], 20 hot
    spheres (radius 2-6 voxels) U[0.6,1.0]."""
    rng = np.random.default_rng(seed)
    vol = rng.uniform(0.0, 0.05, (size, size, size)).astype(np.float32)
    zz, yy, xx = np.ogrid[:size, :size, :size]
    c = size / 2
    body = ((zz - c) / (0.45 * size)) ** 2 + ((yy - c) / (0.35 * size)) ** 2 + ((xx - c) / (0.3 * size)) ** 2 <= 1
    vol[body] = rng.uniform(0.1, 0.4, int(body.sum())).astype(np.float32)
    for _ in range(20):
        r = rng.integers(2, 7)
        ctr = rng.integers(int(0.3 * size), int(0.7 * size), 3)
        sph = (zz - ctr[0]) ** 2 + (yy - ctr[1]) ** 2 + (xx - ctr[2]) ** 2 <= r * r
        vol[sph] = rng.uniform(0.6, 1.0, int(sph.sum())).astype(np.float32)
    return vol


def sliding_bench(model, device, size=256):
    """Config 4: whole-volume sliding-window inference (48^3 windows, overlap 0.5) of a 256^3
    synthetic PET volume, host numpy in -> host prob map out (the reference's contract)."""
    from light_unet.utils import sliding_window_inference_3d, window_positions
    vol = synthetic_pet(size)
    nwin = len(window_positions(size, 48, 24)) ** 3
    sliding_window_inference_3d(vol[:96, :96, :96], model, device=device)   # warm up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prob = sliding_window_inference_3d(vol, model, device=device, window_batch=32)
    dt = time.perf_counter() - t0
    if not np.isfinite(prob).all():
        raise SystemExit("non-finite sliding-window output")
    return {"volume": [size] * 3, "windows": nwin, "seconds": round(dt, 4),
            "ms_per_window": round(1000 * dt / nwin, 4), "window_batch": 32,
            "note": "includes the host->device upload and the prob-map copy back"}


def lesion_bench(device, size=256, reps=5):
    """SURVEY §8f rank 4, post-processing: on the config-4 synthetic PET volume (256^3, 20 hot
    spheres) used as the probability map, Inferencer.extract_bboxes (threshold 0.3, 0.5 cc at 4 mm,
    inferencer.py:62-111) and calculate_lesion_metrics against the spheres (threshold 0.5,
    metrics.py:216-287) on the device (light_unet.lesion, the map already in HBM), beside the
    reference's host path for the same calls (scipy.ndimage.label + the numpy matching, timed on
    this host: the reference's own dependency, not the oracle)."""
    from scipy import ndimage
    from light_unet import lesion
    vol = synthetic_pet(size)
    tgt = (vol >= 0.6).astype(np.float32)
    pv, tv = torch.from_numpy(vol).to(device), torch.from_numpy(tgt).to(device)
    lesion.extract_bboxes(pv, 0.3, 0.5, (4.0, 4.0, 4.0), 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        boxes = lesion.extract_bboxes(pv, 0.3, 0.5, (4.0, 4.0, 4.0), 2)
        met = lesion.calculate_lesion_metrics(pv, tv, threshold=0.5)
    torch.cuda.synchronize()
    dev_ms = 1000 * (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    lab, n = ndimage.label((vol >= 0.3).astype(np.int32))
    sizes = np.bincount(lab.ravel())
    small = sizes < 8
    small[0] = False
    lab[small[lab]] = 0
    lab, n = ndimage.label(lab > 0)
    objs = ndimage.find_objects(lab)
    pl, npred = ndimage.label((vol >= 0.5).astype(np.int32))
    tl, ntgt = ndimage.label(tgt.astype(np.int32))
    ndimage.center_of_mass(np.ones_like(pl, dtype=np.float32), labels=pl, index=np.arange(1, npred + 1))
    np.bincount(pl.ravel().astype(np.int64) * (ntgt + 1) + tl.ravel(), minlength=(npred + 1) * (ntgt + 1))
    host_ms = 1000 * (time.perf_counter() - t0)
    return {"volume": [size] * 3, "device_ms": round(dev_ms, 3), "components": len(boxes),
            "lesion_metrics": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in met.items()},
            "host_scipy_ms": round(host_ms, 1), "host_note": f"scipy.ndimage label x3 + min-size filter + "
            f"find_objects + centres + pair counts, one pass ({len(objs)} boxes)"}


def patches_bench(device, B=4, reps=20):
    """SURVEY §8f rank 4, training patches: a bs-4 batch of 48^3 patches cut and augmented (the
    reference config's flip / rotation / scale / shift / noise probabilities) from the 256^3
    synthetic case resident in HBM (light_unet.patches), beside the reference's per-patch host
    work for the same draws (numpy crop + scipy rotate / zoom, timed on this host)."""
    from scipy import ndimage
    from light_unet.patches import DevicePatchDataset
    aug = {"gaussian_noise": {"enabled": True, "prob": 0.3, "sigma": 0.01},
           "intensity_shift": {"enabled": True, "prob": 0.5, "shift_range": [-0.1, 0.1]},
           "random_flip": {"enabled": True, "prob": 0.5, "axes": [0, 1, 2]},
           "random_rotation": {"enabled": True, "prob": 0.5, "angle_range": [-15, 15],
                               "axes": [[0, 1], [0, 2], [1, 2]]},
           "random_scale": {"enabled": True, "prob": 0.3, "scale_range": [0.9, 1.1]}}
    vol = synthetic_pet(256)
    lab = (vol >= 0.6).astype(np.float32)
    ds = DevicePatchDataset([(vol, lab)], (48, 48, 48), 0.5, aug, seed=42, device=device)
    ds.sample_batch(B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    draws = []
    for _ in range(reps):
        ds.sample_batch(B)
        draws.extend(ds.last_draws)
    torch.cuda.synchronize()
    dev_ms = 1000 * (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for ci, c, d in draws[:8]:
        z, y, x = (max(0, v - 24) for v in c)
        img, lb = vol[z:z + 48, y:y + 48, x:x + 48], lab[z:z + 48, y:y + 48, x:x + 48]
        pad = [(0, 48 - n) for n in img.shape]
        img, lb = np.pad(img, pad), np.pad(lb, pad)
        if d.flip_axis >= 0:
            img = np.flip(img, d.flip_axis).copy()
        if d.rot_axes is not None:
            img = ndimage.rotate(img, d.angle, axes=d.rot_axes, reshape=False, order=1, mode="constant")
            lb = ndimage.rotate(lb, d.angle, axes=d.rot_axes, reshape=False, order=0, mode="constant")
        if d.scale is not None:
            img = ndimage.zoom(img, d.scale, order=1, mode="constant")
            lb = ndimage.zoom(lb, d.scale, order=0, mode="constant")
    host_ms = 1000 * (time.perf_counter() - t0) / 8 * B
    return {"batch": B, "patch": [48, 48, 48], "device_ms_per_batch": round(dev_ms, 3),
            "host_scipy_ms_per_batch": round(host_ms, 1),
            "note": "device: host RNG draws + one l3u_aug_patches launch pair; host: crop + scipy "
                    "rotate / zoom of the same draws, single thread, per batch of the same size"}


def config5_bench(device, world, rank, steps=20, warmup=5, bs=4, size=64, enc=(32, 64, 128, 256)):
    """encoder 32->64->128->256 (812,284 parameters), 64^3 patches, bs 4
    per GPU, the reference's step-based mixed-domain epoch (trainer.py:260-347) with
    dlbcl_steps_ratio 1.0: the FL stream's steps, then as many DLBCL steps, two synthetic
    streams seeded 42 and 43 (loader.py:37 seed+1; rank r adds 1000 r).  Graph-replayed step on
    EVERY rank (data parallel over the job's GPUs, same exchange as the headline step); time =
    max over ranks between barrier + synchronize, throughput = all ranks' patches / time."""
    from light_unet.models.unet3d import Lightweight3DUNet
    from light_unet.train_step import TrainStep
    torch.manual_seed(42)
    model = Lightweight3DUNet(encoder_channels=list(enc), dropout_p=0.1).to(device).train()
    if world > 1:
        dist.broadcast(model.flat_parameters(), 0)
    step = TrainStep(model, {"alpha": 0.7, "beta": 0.3, "gamma": 0.75}, lr=1e-4, weight_decay=1e-5)
    streams = []
    for seed in (42, 43):   # FL, DLBCL
        rng = np.random.default_rng(seed + 1000 * rank)
        x = torch.from_numpy(rng.random((bs, 1, size, size, size), dtype=np.float32)).to(device)
        t = torch.from_numpy((rng.random((bs, 1, size, size, size)) > 0.97).astype(np.float32)).to(device)
        streams.append((x, t))
    xs, ts = streams[0][0].clone(), streams[0][1].clone()
    step.capture(xs, ts, warmup=2)
    half = steps // 2

    def run(i, n):
        src = streams[0] if i < n // 2 else streams[1]   # FL stage, then the DLBCL stage
        xs.copy_(src[0], non_blocking=True)
        ts.copy_(src[1], non_blocking=True)
        return step.replay()

    for i in range(warmup):
        run(i, warmup)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = run(i, steps)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    lv = float(loss.item())
    if not np.isfinite(lv):
        raise SystemExit(f"config 5: non-finite loss {lv}")
    return {"workload": f"Lightweight3DUNet {'->'.join(map(str, enc))} train step, {size}^3, bs {bs}/GPU, "
                        f"step-based FL ({half} steps) then DLBCL ({steps - half} steps)",
            "params": int(model.flat_parameters().numel()), "n_gpus": world,
            "patches_per_s": round(world * steps * bs / dt, 2),
            "patches_per_s_per_gpu": round(steps * bs / dt, 2),
            "ms_per_step": round(1000 * dt / steps, 4), "final_loss": round(lv, 6)}


def grouped_bench(device, steps=10, warmup=3, bs=4, size=48):
    """The use_depthwise_separable=False network family on this GPU: the
    grouped model (GroupedConv3d groups 8; the first block dense, unet3d.py:163-167; 391,521
    parameters) on the config-2 workload (48^3, bs 4, fp32), graph-replayed train step."""
    from light_unet.models.unet3d import Lightweight3DUNet
    from light_unet.train_step import TrainStep
    torch.manual_seed(42)
    model = Lightweight3DUNet(dropout_p=0.1, use_depthwise_separable=False).to(device).train()
    # rank-local (no exchange): this leg runs on rank 0 only
    step = TrainStep(model, {"alpha": 0.7, "beta": 0.3, "gamma": 0.75}, lr=1e-4, weight_decay=1e-5,
                     distributed=False)
    rng = np.random.default_rng(42)
    xs = torch.from_numpy(rng.random((bs, 1, size, size, size), dtype=np.float32)).to(device)
    ts = torch.from_numpy((rng.random((bs, 1, size, size, size)) > 0.97).astype(np.float32)).to(device)
    step.capture(xs, ts, warmup=2)
    for _ in range(warmup):
        step.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step.replay()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lv = float(loss.item())
    if not np.isfinite(lv):
        raise SystemExit(f"grouped model: non-finite loss {lv}")
    return {"workload": f"Lightweight3DUNet use_depthwise_separable=False (groups 8) train step, "
                        f"{size}^3, bs {bs}", "params": int(model.flat_parameters().numel()),
            "patches_per_s_per_gpu": round(steps * bs / dt, 2),
            "ms_per_step": round(1000 * dt / steps, 4), "final_loss": round(lv, 6)}


def dropin_bench(device, steps=20, warmup=5, bs=4, size=48, dropout=0.1):
    """The drop-in path l3u_plugin.install() gives the reference Trainer (trainer.py:222-234):
    model(x) -> FocalTverskyLoss -> zero_grad -> backward (per-parameter autograd) ->
    torch.optim.AdamW.step -> loss.item() (a host sync every step), eager, one GPU."""
    from light_unet.models.losses import FocalTverskyLoss
    from light_unet.models.unet3d import Lightweight3DUNet
    torch.manual_seed(42)
    model = Lightweight3DUNet(dropout_p=dropout).to(device).train()
    crit = FocalTverskyLoss()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5)
    rng = np.random.default_rng(42)
    x = torch.from_numpy(rng.random((bs, 1, size, size, size), dtype=np.float32)).to(device)
    t = torch.from_numpy((rng.random((bs, 1, size, size, size)) > 0.97).astype(np.float32)).to(device)

    def one():
        loss = crit(model(x), t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.item()
    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        lv = one()
    dt = time.perf_counter() - t0
    return {"workload": "drop-in autograd step (model -> FocalTversky -> backward -> torch AdamW -> "
                        f"loss.item()), {size}^3, bs {bs}, eager", "dropin_step_ms": round(1000 * dt / steps, 4),
            "patches_per_s": round(steps * bs / dt, 2), "final_loss": round(lv, 6)}


def bf16_bench(device, args, enc, world, rank, pool):
    """BASELINE config 3: the same step with bf16 activation storage (fp32 master weights, AdamW
    state, gradients and accumulation), graph-replayed, same pool and exchange as the headline;
    with the roofline of its dominant call (the _bf16 depthwise backward)."""
    from light_unet import _native as nat
    from light_unet.models.unet3d import Lightweight3DUNet
    from light_unet.train_step import TrainStep
    torch.manual_seed(42)
    model = Lightweight3DUNet(encoder_channels=list(enc), dropout_p=args.dropout).to(device).train()
    if world > 1:
        dist.broadcast(model.flat_parameters(), 0)
    step = TrainStep(model, {"alpha": 0.7, "beta": 0.3, "gamma": 0.75}, lr=1e-4, weight_decay=1e-5,
                     ftl_mode=args.ftl_mode, dtype=torch.bfloat16)
    xs, ts = [b[0] for b in pool], [b[1] for b in pool]
    for i in range(2):
        step(xs[i], ts[i])
    torch.cuda.synchronize()
    rec = StepRecorder()
    restore = rec.wrap(nat, model.engine)
    step(xs[2], ts[2])
    torch.cuda.synchronize()
    restore()
    orig = rec.orig
    N, S, cdom = args.batch, args.size ** 3, 2 * enc[0]
    dom = [(n, a) for n, a in rec.calls if n == "l3u_dw3_bwd_bf16" and a[-5] == cdom and a[-4] == args.size]
    dom_ms = StepRecorder.time_calls(orig, dom[:1], reps=50)[0] if dom else None
    xt = pool[0].clone()
    step.capture(xt[0], xt[1], warmup=2)
    for i in range(args.warmup):
        xt.copy_(pool[i % 8], non_blocking=True)
        step.replay()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        xt.copy_(pool[i % 8], non_blocking=True)
        loss = step.replay()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    lv = float(loss.item())
    if not np.isfinite(lv):
        raise SystemExit(f"bf16 step: non-finite loss {lv}")
    b = dw_bytes(N, cdom, S, e=2, acc=int(bool(dom[0][1][8])) if dom else 0)
    ach = b / (dom_ms * 1e-3) / 1e9 if dom_ms else None
    return {"workload": "same step, bf16 activation storage (fp32 weights / AdamW / gradients / "
                        "accumulation), graph-replayed", "n_gpus": world,
            "patches_per_s": round(world * args.batch * args.steps / dt, 2),
            "ms_per_step": round(1000 * dt / args.steps, 4), "launches": len(rec.calls),
            "final_loss": round(lv, 6),
            "roofline": {"kernel": f"l3u_dw3_bwd_bf16 [{N},{cdom},{args.size}^3]", "bound": "hbm",
                         "algorithmic_bytes": b, "avg_launch_ms": round(dom_ms, 5) if dom_ms else None,
                         "achieved": round(ach, 1) if ach else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBS, 4) if ach else None}}


def exchange_probe(timeout=240):
    """The world > 1 step's exchange on ONE GPU (tools/rccl_probe.py in a child process: a
    one-rank RCCL group; the single-graph step vs the three graph segments with eager RCCL
    all-reduces vs the all-reduces captured in the graph).  exchange_us = segmented (captured)
    step minus single-graph step: what the data-parallel protocol adds per step before any link
    time."""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_probe.py"), d,
                                str(_free_port())], capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            return {"error": f"timeout after {timeout} s"}
        if r.returncode != 0:
            return {"error": (r.stderr or r.stdout)[-600:]}
        with open(os.path.join(d, "rccl.json")) as f:
            return json.load(f)


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as ONE child process
    (`python -m torch.distributed.run --nproc-per-node N bench.py ...`, rendezvous on
    127.0.0.1), relay its output and return its exit code.  This process never touches the GPU
    (no torch.cuda call before or after), so the child owns every device."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}",
           os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "16")
    return subprocess.run(cmd, env=env).returncode


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one process per GPU")
    dev_index = 0 if args.one_device else local
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        if args.dist_backend == "nccl":   # RCCL over xGMI
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(args.dist_backend)
    enc = tuple(int(c) for c in args.enc.split(","))

    from light_unet import _native as nat
    from light_unet.models.unet3d import Lightweight3DUNet
    from light_unet.train_step import TrainStep

    torch.manual_seed(42)
    model = Lightweight3DUNet(encoder_channels=list(enc), dropout_p=args.dropout).to(device).train()
    if world > 1:   # identical initial weights on every rank (DDP semantics)
        dist.broadcast(model.flat_parameters(), 0)
    step = TrainStep(model, {"alpha": 0.7, "beta": 0.3, "gamma": 0.75}, lr=1e-4, weight_decay=1e-5,
                     ftl_mode=args.ftl_mode,
                     dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    pool = synthetic_pool(8, args.batch, args.size, rank, device)
    xs, ts = [b[0] for b in pool], [b[1] for b in pool]
    xt_static = pool[0].clone()
    x_static, t_static = xt_static[0], xt_static[1]

    # three eager steps come before the capture in every run, so the timed steps start from the
    # same parameters, AdamW state and Dropout3d counter with and without --full
    for i in range(2):
        step(xs[i % 8], ts[i % 8])
    torch.cuda.synchronize()
    if args.full:
        # roofline leg (instrumented): every C-ABI call of the third step recorded at its real
        # shapes and buffers; the dominant call and the depthwise / GEMM families re-timed from
        # the record
        rec = StepRecorder()
        restore = rec.wrap(nat, model.engine)
    step(xs[2], ts[2])
    torch.cuda.synchronize()
    if args.full:
        restore()
        seg_items_from(model.engine)
        orig = rec.orig
        cdom = 2 * enc[0]      # up3.res_block conv1.depthwise: [N, 2*c0, D^3] backward
        dom_name = "l3u_dw3_bwd" + ("_bf16" if args.dtype == "bf16" else "")
        dom_calls = [(n, a) for n, a in rec.calls if n == dom_name and a[-5] == cdom and a[-4] == args.size]
        dom_ms = StepRecorder.time_calls(orig, dom_calls[:1], reps=50)[0] if dom_calls else None
        fams = family_rooflines(orig, rec.calls) if rank == 0 else None
        n_launch_calls = len(rec.calls)
        if args.dump_calls and rank == 0:
            with open(args.dump_calls, "w") as f:
                json.dump([dict(zip(("name", "family", "label", "bytes"),
                                    (n,) + (call_bytes(n, a) or (None, None, None)))) for n, a in rec.calls], f)
        rec = None   # releases the recorded step's buffers

    if args.no_graph:
        def run(i):
            return step(xs[i % 8], ts[i % 8])
    else:
        step.capture(x_static, t_static, warmup=2)

        def run(i):
            xt_static.copy_(pool[i % 8], non_blocking=True)   # the next batch: one D2D copy
            return step.replay()

    for i in range(args.warmup):
        run(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = run(args.warmup + i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    final_loss = float(loss.item())
    if not np.isfinite(final_loss):
        raise SystemExit(f"non-finite loss {final_loss}")
    if args.dump_outputs and rank == 0:
        # what the step hands its caller: the returned loss and, in place, the updated flat
        # parameters and the flat gradient of the last batch
        dump_outputs(args.dump_outputs, {"loss": loss, "params": step.flat, "grads": step.gflat})

    out = None
    if rank == 0:
        out = {
            "metric": METRIC,
            "value": round(world * args.batch * args.steps / elapsed, 2),
            "unit": "patches/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1000 * elapsed / args.steps, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic (x~U[0,1), target Bernoulli(0.03); random-init weights, seed 42)",
            "config": {"workload": f"Lightweight3DUNet {'->'.join(map(str, enc))} train step "
                                   f"(fwd+FocalTversky+bwd+AdamW), {args.size}^3 patches",
                       "batch_per_gpu": args.batch, "global_batch": args.batch * world,
                       "patch": [args.size] * 3, "dropout_p": args.dropout,
                       "ftl_mode": args.ftl_mode,
                       "parallelism": f"dp{world}" if world > 1 else "single",
                       "collectives": (("captured in the step graph" if step.capture_collectives
                                        else "eager between graph segments") if step.exchange
                                       else None),
                       "graph": not args.no_graph},
            "final_loss": round(final_loss, 6),
        }
    if args.full:
        side = side_legs(args, enc, model, pool, device, world, rank,
                         dom_calls, dom_ms, fams, n_launch_calls)
        if rank == 0:
            out.update(side)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return out


def side_legs(args, enc, model, pool, device, world, rank, dom_calls, dom_ms, fams, n_launch_calls):
    """Everything a --full run reports beside the headline step (after it; the `--no-*` options
    drop single legs).  Every rank runs the data-parallel legs; the result keys on rank 0, else
    None."""
    N, S, cdom = args.batch, args.size ** 3, 2 * enc[0]
    sliding = sliding_bench(model, device) if (rank == 0 and not args.no_sliding) else None
    cfg5 = config5_bench(device, world, rank) if not args.no_config5 else None   # every rank
    if cfg5 is not None:
        cfg5["roofline_in_step"] = instep_evidence("c5", None)
        cfg5["step_traffic"] = step_traffic_evidence("c5", cfg5.get("ms_per_step"))
    cfg5 = cfg5 if rank == 0 else None
    grouped = grouped_bench(device) if (rank == 0 and not args.no_grouped) else None
    bf16 = bf16_bench(device, args, enc, world, rank, pool) if (args.dtype == "fp32" and not args.no_bf16) else None
    dropin = dropin_bench(device) if (rank == 0 and not args.no_dropin) else None
    lesion_r = lesion_bench(device) if (rank == 0 and not args.no_data) else None
    patches_r = patches_bench(device) if (rank == 0 and not args.no_data) else None
    exch = exchange_probe() if (world == 1 and not args.no_exchange) else None
    fwd1 = fwd_ms_per_patch(model, 1, args.size, device) if rank == 0 else None
    fwd4 = fwd_ms_per_patch(model, args.batch, args.size, device) if rank == 0 else None
    if rank != 0:
        return None
    dacc = int(bool(dom_calls[0][1][8])) if dom_calls else 0   # accumulates into d(input)
    dbytes = dw_bytes(N, cdom, S, e=2 if args.dtype == "bf16" else 4, acc=dacc)
    achieved = dbytes / (dom_ms * 1e-3) / 1e9 if dom_ms else None
    traffic, traffic_src, traffic_tree = pmc_traffic(N, cdom, args.size, dacc)
    out = {
        "fwd_ms_per_patch": {"bs1": round(fwd1, 4), f"bs{args.batch}": round(fwd4, 4)},
        "sliding_window_256": sliding,
        "config5": cfg5,
        "grouped_1gpu": grouped,
        "bf16": bf16,
        "dropin": dropin,
        "lesion_256": lesion_r,
        "patches": patches_r,
        "launches_per_step": n_launch_calls,
        "exchange": exch,
        "roofline": {
            "kernel": f"l3u_dw3_bwd [{N},{cdom},{args.size}^3] (up3.res_block.conv1.depthwise "
                      "backward: one single-pass launch, data and weight gradients from one "
                      "LDS-DMA-staged read of dZ and A"
                      + (", adding to the shortcut's d(input))" if dacc else ")"),
            "bound": "hbm",
            "achieved": round(achieved, 1) if achieved else None,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4) if achieved else None,
            "traffic": traffic,
            "traffic_source": traffic_src,
            "traffic_tree_matches": traffic_tree,
            "algorithmic_bytes": dbytes,
            "avg_launch_ms": round(dom_ms, 5) if dom_ms else None,
            "cache_exceeding": dw_bwd_cache_exceeding(device),
            "in_step": instep_evidence(
                "c5" if enc == (32, 64, 128, 256) and args.size == 64 else args.dtype, n_launch_calls),
            "depthwise": fams["dw"],
            "gemm": dict(fams["gemm"], calls=sorted(fams["gemm"]["calls"], key=lambda r: -r["us"])[:5],
                         mfma=gemm_mfma_evidence()),
            # the InstanceNorm / block-tail launches and the out_conv + loss launches
            "norm": dict(fams["norm"], calls=sorted(fams["norm"]["calls"], key=lambda r: -r["us"])[:5]),
            "io": fams["io"],
        },
    }
    if world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args, enc)
    return out


if __name__ == "__main__":
    main()
