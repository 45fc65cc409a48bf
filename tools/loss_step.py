"""Cost of the loss family in the graph-replayed training step: config 2 (bs 4 x 48^3, dropout
0.1, fp32) with FocalTverskyLoss, CombinedLoss (0.8 / 0.2) and DiceLoss, timed with bench.py's
protocol (resident batch pool, one D2D staging copy + one graph replay per step, perf_counter
around `steps` replays between synchronisations), the three steps interleaved round by round on
one box so that they share its clocks and temperature.

    python tools/loss_step.py [--steps 60] [--warmup 10] [--rounds 5]
        one JSON line: per loss the ms/step of every round and their median, the ratio of the
        medians to the FocalTversky step of the same run, and the C-ABI launches per step.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \\
        python tools/loss_step.py --only combined --rounds 1 --steps 40
    python tools/loss_step.py --outconv-trace DIR/.../run_kernel_trace.csv --steps 40
        in-step duration of the two out_conv launches: mean over the last `steps` occurrences of
        outconv_fwd_kernel / outconv_bwd_kernel in the trace (the graph replays).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "light-3d-unet-front_amd")):
    sys.path.insert(0, p)

LOSSES = {
    "ftl": {"name": "FocalTverskyLoss", "alpha": 0.7, "beta": 0.3, "gamma": 0.75},
    "combined": {"name": "FocalTverskyLoss", "alpha": 0.7, "beta": 0.3, "gamma": 0.75,
                 "use_combined_loss": True,
                 "combined_loss_weights": {"focal_tversky": 0.8, "bce": 0.2}},
    "dice": {"name": "DiceLoss"},
}


def outconv_from_trace(path, steps):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for key in ("outconv_fwd_kernel", "outconv_bwd_kernel"):
        d = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows
             if key in r["Kernel_Name"]][-steps:]
        out[key + "_us"] = round(sum(d) / len(d) / 1e3, 3) if d else None
        out[key + "_n"] = len(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--only", default=None, choices=sorted(LOSSES))
    ap.add_argument("--outconv-trace", default=None, metavar="CSV")
    args = ap.parse_args()
    if args.outconv_trace:
        print(json.dumps(outconv_from_trace(args.outconv_trace, args.steps)))
        return

    import numpy as np
    import torch
    from light_unet import _native as nat
    from light_unet.models.unet3d import Lightweight3DUNet
    from light_unet.train_step import TrainStep

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pool = []
    for i in range(8):   # bench.py synthetic_pool
        rng = np.random.default_rng(42 + i)
        shape = (args.batch, 1, args.size, args.size, args.size)
        x = rng.random(shape, dtype=np.float32)
        t = (rng.random(shape) > 0.97).astype(np.float32)
        pool.append(torch.from_numpy(np.stack([x, t])).to(dev))
    names = [args.only] if args.only else list(LOSSES)
    runs = {}
    for name in names:
        torch.manual_seed(42)
        model = Lightweight3DUNet(dropout_p=args.dropout).to(dev).train()
        step = TrainStep(model, LOSSES[name], lr=1e-4, weight_decay=1e-5)
        for i in range(2):
            step(pool[i][0], pool[i][1])
        calls, real = [], nat.call
        nat.call = lambda n, *a: (calls.append(n), real(n, *a))[1]
        try:
            step(pool[2][0], pool[2][1])
        finally:
            nat.call = real
        torch.cuda.synchronize()
        xt = pool[0].clone()
        step.capture(xt[0], xt[1], warmup=2)
        runs[name] = {"step": step, "xt": xt, "ms": [], "launches": len(calls),
                      "outconv_calls": [c for c in calls if "outconv" in c]}

    def replay(r, i):
        r["xt"].copy_(pool[i % 8], non_blocking=True)
        return r["step"].replay()

    for name in names:
        for i in range(args.warmup):
            replay(runs[name], i)
    torch.cuda.synchronize()
    k = args.warmup
    for _ in range(args.rounds):
        for name in names:
            r = runs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                loss = replay(r, k + i)
            torch.cuda.synchronize()
            r["ms"].append(round(1000 * (time.perf_counter() - t0) / args.steps, 4))
            r["final_loss"] = round(float(loss.item()), 6)
        k += args.steps
    out = {"workload": f"bs {args.batch} x {args.size}^3, dropout {args.dropout}, fp32, graph replay",
           "steps": args.steps, "rounds": args.rounds}
    for name in names:
        r = runs[name]
        out[name] = {"ms_per_step": r["ms"], "median_ms": round(statistics.median(r["ms"]), 4),
                     "launches": r["launches"], "outconv_calls": r["outconv_calls"],
                     "final_loss": r["final_loss"]}
    if "ftl" in out:
        for name in names:
            out[name]["vs_ftl"] = round(out[name]["median_ms"] / out["ftl"]["median_ms"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
