"""Device times of the resegmentation by an uptake threshold (light_unet/resegment.py,
csrc/resegment.hip) on the synthetic case of tools/quantify_bench.py: 40 ellipsoids with gamma
noise, 6 units hotter inside, in 204 x 204 x 450 voxels at 4 mm and as 400 x 400 x 600 at
(3, 2.04, 2.04) mm where the memory allows (--no-large skips it).  The seeds are the ellipsoids.

    python tools/resegment_bench.py [--repeat 10] [--out profiles/resegment_bench.json] [--no-host]
    python tools/resegment_bench.py --ab-parent DIR [--ab-rounds 3]

Both methods ("fixed" 4.0 and "relative" 0.41) at grow_mm = 20.  Medians of --repeat runs after a
warm-up, HIP events around the native calls, per seed path: the LDS path is one l3u_rs_grow launch
over the seeds whose box fits; the tiled path is resegment._grow for the other seeds: l3u_rs_grow's
build, the l3u_rs_sweep launches with the reads of their counters between them, l3u_rs_commit, and
the zeroing, uploads and download around them.  Where every box fits the LDS the tiled path has no
seed, so every seed is also run once the tiled way (max_lds_bytes = 16).  With them the number of
seeds on each path, the largest box and the largest sweep (or launch) count; a host clock (ending in a
device synchronise) around a whole resegment_lesions call on device-resident inputs, the labelling
of the seeds included; the same result from numpy and scipy.ndimage.label per box on the host
(a numpy breadth-first search where scipy does not import), timed once, and the number of voxels
in which the two label maps differ, which must be 0.  Needs a GPU: no fallback.

--ab-parent DIR: the untouched path.  DIR holds another build of this repository (the parent
commit); tools/quantify_bench.py's 204 x 204 x 450 case runs in child processes alternating between
DIR and this tree, and the medians of a whole lesion_uptake call (no resegment) are reported side
by side with each tree's own spread over the rounds."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-3d-unet-front_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from light_unet import _native as nat          # noqa: E402
from light_unet import lesion                  # noqa: E402
from light_unet import quantify as QT          # noqa: E402
from light_unet import resegment as RS         # noqa: E402
from quantify_bench import uptake_of           # noqa: E402
from surface_bench import CASES, blobs         # noqa: E402

GROW_MM = 20.0
FORCE_TILED = 16   # max_lds_bytes at which no box fits the LDS
METHODS = (("fixed", 4.0), ("relative", 0.41))


def median_ms(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def time_lds(up, seeds, items, thr, shape, repeat):
    """HIP events around l3u_rs_grow alone, over the LDS seeds of the item table (the map zeroed and
    the tables uploaded outside the events)."""
    dev, n = up.device, len(items)
    items_d, thr_d = torch.from_numpy(items).to(dev), torch.from_numpy(thr).to(dev)
    own = torch.empty(shape, dtype=torch.int32, device=dev)
    reached = torch.empty(n, dtype=torch.int64, device=dev)
    sweeps = torch.empty(n, dtype=torch.int32, device=dev)
    ms = []
    for _ in range(repeat + 2):
        own.zero_()
        reached.zero_()
        sweeps.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        nat.call("l3u_rs_grow", up.data_ptr(), seeds.data_ptr(), None, 0, items_d.data_ptr(),
                 thr_d.data_ptr(), n, 1, own.data_ptr(), reached.data_ptr(), sweeps.data_ptr(), None,
                 0, None, None, 0, *shape, nat.stream())
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return median_ms(ms[2:]), reached.cpu().numpy(), sweeps.cpu().numpy()


def time_tiled(up, seeds, items, tiles, aoff, words, thr, shape, repeat, max_lds_bytes):
    """HIP events around resegment._grow for an item table whose LDS seeds are marked away (path
    2: skipped): zeroing the map, the table uploads, l3u_rs_grow's build, the l3u_rs_sweep launches
    with the reads of their counters, l3u_rs_commit and the download of the counts."""
    ms = []
    for _ in range(repeat + 2):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        own, reached, sweeps = RS._grow(up, seeds, None, items, tiles, aoff, words, thr, True,
                                        max_lds_bytes, shape)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return median_ms(ms[2:]), reached, sweeps, own


def host_resegment(up, lab, boxes, thr):
    """The label map (smallest label first) from numpy / scipy, box by box."""
    try:
        from scipy import ndimage as ndi
        how = "scipy.ndimage.label per box"
    except ImportError:
        ndi, how = None, "numpy breadth-first search per box"
    t0 = time.perf_counter()
    out = np.zeros(lab.shape, dtype=np.int32)
    for i in reversed(range(len(boxes))):
        z0, z1, y0, y1, x0, x1 = (int(v) for v in boxes[i])
        box = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        cand = up[box].astype(np.float64) >= thr[i]
        start = cand & (lab[box] == i + 1)
        if ndi is not None:
            comp, _ = ndi.label(cand)
            hit = np.unique(comp[start])
            r = np.isin(comp, hit[hit > 0])
        else:
            r, frontier = start.copy(), start.copy()
            while frontier.any():
                nb = np.zeros_like(frontier)
                nb[1:] |= frontier[:-1]
                nb[:-1] |= frontier[1:]
                nb[:, 1:] |= frontier[:, :-1]
                nb[:, :-1] |= frontier[:, 1:]
                nb[:, :, 1:] |= frontier[:, :, :-1]
                nb[:, :, :-1] |= frontier[:, :, 1:]
                frontier = nb & cand & ~r
                r |= frontier
        out[box][r] = i + 1
    return out, time.perf_counter() - t0, how


def path_record(ext, mine, reached, sweeps, t):
    big = int(np.argmax(np.where(mine, ext.prod(axis=1), -1)))
    return {"largest_box": ext[big].tolist(),
            "largest_box_words": int(ext[big, 0] * ext[big, 1] * ((ext[big, 2] + 63) // 64)),
            "largest_sweeps": int(sweeps[mine].max()), "reached_voxels": int(reached[mine].sum()),
            "native_calls": t}


def case(shape, spacing, repeat, host):
    dev = torch.device("cuda", torch.cuda.current_device())
    mask = blobs(shape, spacing, dev)
    up = uptake_of(mask)
    comp = lesion.label(mask, 0.5)
    seeds = comp.labels.contiguous()
    n = comp.num
    pad = RS.box_padding(GROW_MM, spacing)
    boxes = RS.seed_boxes(comp.stats, pad, shape)
    items, tiles, aoff, words = RS._plan(boxes, 0)
    ext = boxes[:, 1::2] - boxes[:, 0::2]
    rec = {"shape": list(shape), "spacing": list(spacing), "voxels": mask.numel(), "seeds": n,
           "seed_voxels": int(comp.sizes().sum()), "grow_mm": GROW_MM, "padding_voxels": list(pad),
           "arena_bytes": int(words) * 8, "tiles": int(len(tiles))}
    seed_max = QT._reduce(up, seeds, None, comp.stats, shape)[:, 2].astype(np.float32)
    up_h = lab_h = None
    for method, value in METHODS:
        thr = RS.thresholds_for(method, value, seed_max)
        m = {"value": value}
        for path, name in ((0, "lds"), (1, "tiled")):
            mine = items[:, 7] == path
            m[name] = {"seeds": int(mine.sum())}
            if not mine.any():
                continue
            only = items.copy()
            only[~mine, 7] = 2
            if path == 0:
                t, reached, sweeps = time_lds(up, seeds, only, thr, shape, repeat)
            else:
                t, reached, sweeps, _ = time_tiled(up, seeds, only, tiles, aoff, words, thr, shape,
                                                   repeat, 0)
            m[name].update(path_record(ext, mine, reached, sweeps, t))
        # every seed forced the tiled way: the same regions through the arena
        items_t, tiles_t, aoff_t, words_t = RS._plan(boxes, FORCE_TILED)
        t, reached, sweeps, own_t = time_tiled(up, seeds, items_t, tiles_t, aoff_t, words_t, thr, shape,
                                               repeat, FORCE_TILED)
        m["tiled_forced"] = {"max_lds_bytes": FORCE_TILED, "seeds": n, "tiles": int(len(tiles_t)),
                             "arena_bytes": int(words_t) * 8}
        m["tiled_forced"].update(path_record(ext, np.ones(n, dtype=bool), reached, sweeps, t))
        calls, calls_comp = [], []
        for _ in range(repeat + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rs = RS.resegment_lesions(up, mask, spacing, method=method, value=value, grow_mm=GROW_MM)
            torch.cuda.synchronize()
            calls.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            RS.resegment_lesions(up, comp, spacing, method=method, value=value, grow_mm=GROW_MM)
            torch.cuda.synchronize()
            calls_comp.append((time.perf_counter() - t0) * 1e3)
        m["resegment_lesions_call"] = median_ms(calls[1:])
        m["resegment_lesions_call_given_components"] = median_ms(calls_comp[1:])
        m["result"] = {"regions": rs.components.num, "voxels": int(rs.components.sizes().sum()),
                       "below_threshold": int((rs.status == 1).sum()),
                       "absorbed": int((rs.status == 2).sum())}
        if host:
            if up_h is None:
                up_h, lab_h = up.cpu().numpy(), seeds.cpu().numpy()
            ref, secs, how = host_resegment(up_h, lab_h, boxes, thr)
            keep = np.zeros(n + 1, dtype=np.int32)
            keep[rs.seed_label] = np.arange(1, len(rs.seed_label) + 1)
            back = np.zeros(n + 1, dtype=np.int32)
            back[1:] = np.arange(n, 0, -1)    # the forced tiled run's map holds n + 1 - label
            m["host"] = {"how": how, "total_s": secs,
                         "differing_voxels": int((keep[ref] != rs.components.numpy()).sum()),
                         "differing_voxels_tiled_forced": int((ref != back[own_t.cpu().numpy()]).sum()),
                         "regions": int(len(np.unique(ref)) - 1)}
        rec[method] = m
    return rec


def ab(parent, rounds, repeat):
    """lesion_uptake without resegment, this tree against `parent`, child processes alternating."""
    name = CASES[0][0]
    runs = {"parent": [], "this": []}
    for _ in range(rounds):
        for who, tree in (("parent", parent), ("this", ROOT)):
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, "q.json")
                subprocess.run([sys.executable, os.path.join(tree, "tools", "quantify_bench.py"),
                                "--no-host", "--only", name, "--repeat", str(repeat), "--out", out],
                               check=True, stdout=subprocess.DEVNULL, timeout=300)
                with open(out) as f:
                    runs[who].append(json.load(f)[name]["lesion_uptake_call"]["median_ms"])
    res = {"case": name, "what": "median ms of a whole lesion_uptake call (no resegment) per child "
           "process, parent commit and this tree alternating on one box", "rounds": rounds}
    for who, v in runs.items():
        res[who] = {"medians_ms": v, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    res["this_over_parent"] = res["this"]["median_ms"] / res["parent"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip numpy / scipy on the host")
    ap.add_argument("--no-large", action="store_true", help="skip the 400 x 400 x 600 case")
    ap.add_argument("--ab-parent", default=None, help="a built tree of the parent commit")
    ap.add_argument("--ab-rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resegment_bench needs a ROCm GPU")
    if a.ab_parent:
        res = {"device": torch.cuda.get_device_name(0),
               "lesion_uptake_untouched": ab(os.path.abspath(a.ab_parent), a.ab_rounds, a.repeat)}
    else:
        res = {"device": torch.cuda.get_device_name(0), "repeat": a.repeat,
               "note": "one run on one box; no speed gate"}
        for name, shape, spacing in CASES:
            if a.no_large and name != CASES[0][0]:
                continue
            try:
                res[name] = case(shape, spacing, a.repeat, not a.no_host)
            except torch.cuda.OutOfMemoryError:
                res[name] = {"skipped": "out of device memory"}
                torch.cuda.empty_cache()
            print(name, json.dumps(res[name]), flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
