"""Lesion post-processing on the MI355X: connected components, lesion matching, lesion metrics and
bounding boxes, mirroring the reference's host functions

    get_connected_components   light_unet/models/metrics.py:38-63
    match_components           light_unet/models/metrics.py:127-213
    calculate_lesion_metrics   light_unet/models/metrics.py:216-287
    calculate_metrics          light_unet/models/metrics.py:306-404
    extract_bboxes             light_unet/core/inferencer.py:62-111

with the same signatures, return types and numbering.  The per-voxel work runs in the HIP
kernels of csrc/lesion.hip (include/l3u.h, l3u_ccl_*): labelling (scipy.ndimage.label's
6-connectivity and first-encounter numbering), per-component sizes / coordinate sums / bounding
boxes / peak probability (exact integer atomics), and the pairwise overlap counts of two
labellings.  What stays on the host is O(components): the greedy matching loop and the final
ratios, written as the reference writes them so the floats agree bit for bit.  Inputs may be
numpy arrays (uploaded once) or device tensors; there is no CPU fallback.
"""
import math

import numpy as np
import torch

from . import _native as nat

# stats columns (csrc/lesion.hip)
_SIZE, _SUM, _MIN, _MAX, _PMAX = 0, slice(1, 4), slice(4, 7), slice(7, 10), 10


def _device():
    if not torch.cuda.is_available():
        raise nat.NativeError("lesion post-processing runs on the ROCm device; no GPU is visible "
                              "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _dims(shape):
    """(B, D, H, W, lead4) of a labelled / thresholded array, in ndimage.label's own terms: a
    [D, H, W] volume (B = 1, coordinates z, y, x) or a [B, D, H, W] array labelled as ONE
    4-dimensional array (the batch axis is a fourth face neighbour; the reference's centres keep
    the leading coordinates b, z, y, metrics.py:99-124).  Other ranks are not taken."""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 3:
        return (1,) + shape + (0,)
    if len(shape) == 4:
        return shape + (1,)
    raise ValueError(f"expected a [D, H, W] volume or a [B, D, H, W] array, got shape {shape}")


def _volume(a, dev, keep_f64=False):
    """The array (3- or 4-dimensional, shape kept) as float32 on the device.  keep_f64: a float64
    input stays float64 (the reference thresholds float64 maps in float64)."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    _dims(t.shape)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    dt = torch.float64 if (keep_f64 and t.dtype == torch.float64) else torch.float32
    return t.to(device=dev, dtype=dt).contiguous()


def _foreground(vol, threshold, dev):
    """(volume, threshold) for l3u_ccl_label, which compares in float32.  A float64 map is
    compared in float64 on the device first (`vol >= threshold` as metrics.py:245 /
    inferencer.py:64 evaluate it in numpy), so values between float32(threshold) and threshold
    classify as the reference classifies them; the kernel then labels the 0/1 mask."""
    v = _volume(vol, dev, keep_f64=True)
    if v.dtype == torch.float64:
        return (v >= float(threshold)).to(torch.float32), 0.5
    return v, threshold


class Components:
    """A labelling on the device: `labels` int32 (the input's [D, H, W] or [B, D, H, W] shape),
    `num` components, `stats` uint64 [num, 12] (host) as l3u_ccl_stats_b writes them."""

    def __init__(self, labels, num, stats):
        self.labels, self.num, self.stats = labels, int(num), stats
        self.pmax64 = None   # float64 per-component maxima of a float64 prob map (label(prob=))

    def sizes(self):
        return self.stats[:, _SIZE].astype(np.int64)

    def centers(self):
        """Centres of mass in voxels, scipy.ndimage.center_of_mass's float64 sum / count (the
        three leading coordinates of the array, as metrics.py:99-124 keeps them)."""
        if self.num == 0:
            return np.empty((0, 3), dtype=np.float64)
        return self.stats[:, _SUM].astype(np.float64) / self.stats[:, _SIZE:_SIZE + 1].astype(np.float64)

    def numpy(self):
        return self.labels.cpu().numpy()


def label(vol, threshold=0.5, min_size=0, prob=None):
    """Components of (vol >= threshold); min_size > 0 drops smaller ones and renumbers the rest in
    order (metrics.py:52-61: removing whole components never changes the others' connectivity, so
    ndimage.label of the survivors is the order-preserving rank).  prob: optional volume whose
    per-component maximum lands in stats[:, 10] (float32 bits)."""
    dev = _device()
    v, threshold = _foreground(vol, threshold, dev)
    B, D, H, W, lead4 = _dims(v.shape)
    n = v.numel()
    st = nat.stream()
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    lab = torch.empty(v.shape, dtype=torch.int32, device=dev)
    nch = nat.query("l3u_ccl_nchunks", n)
    cnt = torch.empty(nch + 1, dtype=torch.int32, device=dev)
    nat.call("l3u_ccl_label_b", v.data_ptr(), float(threshold), parent.data_ptr(), lab.data_ptr(),
             cnt.data_ptr(), B, D, H, W, st)
    num = int(cnt[nch].item())
    if num == 0:
        return Components(lab, 0, np.zeros((0, 12), dtype=np.uint64))
    pv = _volume(prob, dev, keep_f64=True) if prob is not None else None
    if pv is not None and tuple(pv.shape) != tuple(v.shape):
        raise ValueError("prob must have the labelled volume's shape")
    pv64 = None
    if pv is not None and pv.dtype == torch.float64:
        # the kernel's per-component maximum is float32; a float64 map keeps its own maximum
        # (float(prob_map[component_mask].max()) in inferencer.py:98), taken below
        pv64, pv = pv, None
    stats = torch.empty(num * 12, dtype=torch.int64, device=dev)
    nat.call("l3u_ccl_stats_b", lab.data_ptr(), None, pv.data_ptr() if pv is not None else None,
             stats.data_ptr(), num, B, D, H, W, lead4, st)
    s = stats.view(num, 12).cpu().numpy().view(np.uint64)
    if min_size > 0:
        keep = s[:, _SIZE] >= min_size
        if not keep.all():
            remap = np.zeros(num + 1, dtype=np.int32)
            remap[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
            num = int(keep.sum())
            rm = torch.from_numpy(remap).to(dev)
            if num == 0:   # every component dropped: the remap pass only clears the labels
                stats = torch.empty(12, dtype=torch.int64, device=dev)
                nat.call("l3u_ccl_stats_b", lab.data_ptr(), rm.data_ptr(), None, stats.data_ptr(), 1,
                         B, D, H, W, lead4, st)
                return Components(lab, 0, np.zeros((0, 12), dtype=np.uint64))
            stats = torch.empty(num * 12, dtype=torch.int64, device=dev)
            nat.call("l3u_ccl_stats_b", lab.data_ptr(), rm.data_ptr(),
                     pv.data_ptr() if pv is not None else None, stats.data_ptr(), num, B, D, H, W,
                     lead4, st)
            s = stats.view(num, 12).cpu().numpy().view(np.uint64)
    c = Components(lab, num, s)
    if pv64 is not None:
        m = torch.full((num + 1,), -math.inf, dtype=torch.float64, device=dev)
        m.scatter_reduce_(0, lab.reshape(-1).long(), pv64.reshape(-1), "amax")
        c.pmax64 = m[1:].cpu().numpy()
    return c


def get_connected_components(mask, min_size=0):
    """metrics.py:38-63: (labeled int32 numpy of the mask's shape, num_components); foreground =
    mask != 0; a [B, D, H, W] mask is labelled as one 4-dimensional array, as ndimage.label does."""
    m = np.asarray(mask) if not isinstance(mask, torch.Tensor) else mask
    fg = (m != 0)
    c = label(fg.astype(np.float32) if isinstance(fg, np.ndarray) else fg.float(), 0.5, min_size)
    return c.numpy(), c.num


def _as_components(lab_or_comp):
    if isinstance(lab_or_comp, Components):
        return lab_or_comp
    dev = _device()
    t = lab_or_comp if isinstance(lab_or_comp, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(lab_or_comp)))
    B, D, H, W, lead4 = _dims(t.shape)
    t = t.to(device=dev, dtype=torch.int32).contiguous()
    num = int(t.max().item()) if t.numel() else 0
    if num == 0:
        return Components(t, 0, np.zeros((0, 12), dtype=np.uint64))
    stats = torch.empty(num * 12, dtype=torch.int64, device=dev)
    nat.call("l3u_ccl_stats_b", t.data_ptr(), None, None, stats.data_ptr(), num, B, D, H, W, lead4,
             nat.stream())
    return Components(t, num, stats.view(num, 12).cpu().numpy().view(np.uint64))


def _intersections(pc, tc):
    """(num_pred + 1, num_target + 1) int64 overlap counts, row / column 0 zero (metrics.py:153-162)."""
    inter = torch.zeros((pc.num + 1) * (tc.num + 1), dtype=torch.int32, device=pc.labels.device)
    nat.call("l3u_ccl_pairs", pc.labels.data_ptr(), tc.labels.data_ptr(), tc.num, inter.data_ptr(),
             pc.labels.numel(), nat.stream())
    return inter.view(pc.num + 1, tc.num + 1).cpu().numpy().astype(np.int64)


def _sizes0(c):
    out = np.zeros(c.num + 1, dtype=np.int64)
    out[1:] = c.sizes()
    return out


def match_components(pred_labeled, target_labeled, iou_threshold=0.1, distance_threshold_mm=10.0,
                     spacing=(4.0, 4.0, 4.0), inter=None):
    """metrics.py:127-213: greedy matching of predicted to target components by IoU or centre
    distance.  Labelled arrays (numpy / device, [D, H, W] or [B, D, H, W]) or Components.
    inter: the (num_pred + 1, num_target + 1) overlap table when the caller has it already (the
    threshold sweep counts every level's overlaps in one launch)."""
    pc, tc = _as_components(pred_labeled), _as_components(target_labeled)
    num_pred, num_target = pc.num, tc.num
    if num_pred == 0 or num_target == 0:
        return [], list(range(1, num_pred + 1)), list(range(1, num_target + 1))
    intersection = _intersections(pc, tc) if inter is None else inter
    pred_sizes, target_sizes = _sizes0(pc), _sizes0(tc)
    union = pred_sizes[:, None] + target_sizes[None, :] - intersection
    iou_matrix = np.divide(intersection, union, out=np.zeros_like(intersection, dtype=np.float32),
                           where=union > 0)
    spacing_arr = np.asarray(spacing, dtype=np.float64)
    pred_centers = pc.centers() * spacing_arr
    target_centers = tc.centers() * spacing_arr
    distance_matrix = np.linalg.norm(pred_centers[:, None, :] - target_centers[None, :, :], axis=2)
    matches = []
    matched_target = np.zeros(num_target, dtype=bool)
    for pid in range(1, num_pred + 1):
        iou_row = iou_matrix[pid, 1:]
        valid = ~matched_target & ((iou_row >= iou_threshold) |
                                   (distance_matrix[pid - 1] <= distance_threshold_mm))
        if not np.any(valid):
            continue
        best = int(np.argmax(np.where(valid, iou_row, -np.inf)))
        matches.append((pid, best + 1))
        matched_target[best] = True
    matched_pred = {p for p, _ in matches}
    return (matches, [i for i in range(1, num_pred + 1) if i not in matched_pred],
            [i for i in range(1, num_target + 1) if not matched_target[i - 1]])


def _squeeze(a):
    if len(a.shape) == 5:
        a = a[:, 0]
    if len(a.shape) == 4 and a.shape[0] == 1:
        a = a[0]
    return a


def _lesion_counts(pc, tc, iou_threshold, distance_threshold_mm, spacing, inter=None):
    if tc.num == 0:
        return (0, pc.num, 0)
    if pc.num == 0:
        return (0, 0, tc.num)
    m, up, ut = match_components(pc, tc, iou_threshold, distance_threshold_mm, spacing, inter)
    return (len(m), len(up), len(ut))


def calculate_lesion_metrics(pred, target, threshold=0.5, min_size_voxels=0, iou_threshold=0.1,
                             distance_threshold_mm=10.0, spacing=(4.0, 4.0, 4.0)):
    """metrics.py:216-287: lesion-wise recall / precision / f1 and tp / fp / fn counts."""
    pred, target = _squeeze(pred), _squeeze(target)
    pc = label(pred, threshold, min_size_voxels)
    tc = label(target, 0.5, min_size_voxels)
    if tc.num == 0:
        if pc.num == 0:
            return {"recall": 1.0, "precision": 1.0, "f1": 1.0, "tp": 0, "fp": 0, "fn": 0}
        return {"recall": 0.0, "precision": 0.0, "f1": 0.0, "tp": 0, "fp": pc.num, "fn": 0}
    if pc.num == 0:
        return {"recall": 0.0, "precision": 0.0, "f1": 0.0, "tp": 0, "fp": 0, "fn": tc.num}
    tp, fp, fn = _lesion_counts(pc, tc, iou_threshold, distance_threshold_mm, spacing)
    recall = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    precision = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    f1 = 2 * (precision * recall) / (precision + recall) if (precision + recall) > 0 else 0.0
    return {"recall": recall, "precision": precision, "f1": f1, "tp": tp, "fp": fp, "fn": fn}


def calculate_metrics(predictions, labels, threshold=0.5, spacing=(4.0, 4.0, 4.0)):
    """metrics.py:306-404: lesion-wise and voxel-wise (DSC micro / macro) metrics over cases.  The
    voxel counts come from the same device labelling (foreground sizes and overlaps)."""
    pred_list, label_list = _case_list(predictions, "predictions"), _case_list(labels, "labels")
    spacings = _spacing_per_case(spacing, len(pred_list))
    for pred, target in zip(pred_list, label_list):   # shapes first: no device work on a bad list
        _dims(_squeeze(np.asarray(pred)).shape)
        _dims(_squeeze(np.asarray(target)).shape)
    smooth = 1e-6
    tot_tp = tot_fp = tot_fn = 0
    inter_sum = union_sum = 0.0
    per_case = []
    for pred, target, sp in zip(pred_list, label_list, spacings):
        pred, target = _squeeze(np.asarray(pred)), _squeeze(np.asarray(target))
        pc, tc = label(pred, threshold), label(target, 0.5)
        ps, ts = int(pc.sizes().sum()), int(tc.sizes().sum())
        inter = int(_intersections(pc, tc).sum()) if pc.num and tc.num else 0
        inter_sum += inter
        union_sum += ps + ts
        per_case.append((2.0 * inter + smooth) / ((ps + ts) + smooth))
        if tc.num == 0:
            tp, fp, fn = (0, 0 if pc.num == 0 else pc.num, 0)
        elif pc.num == 0:
            tp, fp, fn = (0, 0, tc.num)
        else:
            tp, fp, fn = _lesion_counts(pc, tc, 0.1, 10.0, sp)
        tot_tp += tp
        tot_fp += fp
        tot_fn += fn
    n = len(pred_list)
    dsc_micro = (2.0 * inter_sum + smooth) / (union_sum + smooth)
    dsc_macro = np.mean(per_case) if per_case else 0.0
    recall = tot_tp / (tot_tp + tot_fn) if (tot_tp + tot_fn) > 0 else 0.0
    precision = tot_tp / (tot_tp + tot_fp) if (tot_tp + tot_fp) > 0 else 0.0
    f1 = (2 * precision * recall) / (precision + recall) if (precision + recall) > 0 else 0.0
    return {"lesion_wise_recall": recall, "lesion_wise_precision": precision, "lesion_wise_f1": f1,
            "voxel_wise_dsc_micro": dsc_micro, "voxel_wise_dsc_macro": dsc_macro,
            "fp_per_case": tot_fp / n if n > 0 else 0.0, "tp": tot_tp, "fp": tot_fp, "fn": tot_fn,
            "dsc": dsc_micro, "recall": recall, "precision": precision}


# ------------------------------------------------------------------ the threshold sweep
MAX_LEVELS = 32   # csrc/lesion.hip kMaxLv


def level_map(prob, thresholds, mask=None, target=None, want_masked=False):
    """l3u_thr_levels: `prob` (device float32, any shape; * `mask` in float32 when given) against
    the strictly ascending float32 `thresholds` (1..32 of them).  Returns (level uint8 of prob's
    shape, hist int64 device [(K + 1), 2]: voxels per (level, target >= 0.5), masked map or None)."""
    thr = np.ascontiguousarray(thresholds, dtype=np.float32)
    K = int(thr.size)
    if not (1 <= K <= MAX_LEVELS) or not np.all(thr[1:] > thr[:-1]) or not np.all(np.isfinite(thr)):
        raise ValueError(f"thresholds must be 1..{MAX_LEVELS} finite, strictly ascending float32 values")
    nat.require_device(prob, mask, target)
    for t in (prob, mask, target):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()
                              or t.numel() != prob.numel()):
            raise ValueError("level_map takes contiguous float32 device tensors of one size")
    dev = prob.device
    level = torch.empty(prob.shape, dtype=torch.uint8, device=dev)
    hist = torch.empty((K + 1, 2), dtype=torch.int64, device=dev)
    masked = torch.empty_like(prob) if want_masked else None
    thr_d = torch.from_numpy(thr).to(dev)
    nat.call("l3u_thr_levels", prob.data_ptr(), nat.ptr(mask), nat.ptr(target), thr_d.data_ptr(), K,
             level.data_ptr(), hist.data_ptr(), nat.ptr(masked), prob.numel(), nat.stream())
    return level, hist, masked


def label_levels(level, K, k0=0, prob=None, target=None):
    """The K binarisations level >= k0 + k + 1 (k = 0..K-1) of one [D, H, W] level volume
    (level_map), labelled side by side: one l3u_ccl_label_lv, one read-back of the K counts, one
    l3u_ccl_stats_lv and -- with `target` (a Components of the same shape) -- one
    l3u_ccl_pairs_lv, whatever K.  Returns ([Components per level], [overlap table per level] or
    None); every Components is what label(p, thr[k0 + k]) returns (labels are views of one
    [K, D, H, W] tensor; prob lands in stats[:, 10])."""
    D, H, W = (int(v) for v in level.shape)
    n = D * H * W
    K, k0 = int(K), int(k0)
    if not (K >= 1 and k0 >= 0 and k0 + K <= MAX_LEVELS):
        raise ValueError(f"levels {k0}..{k0 + K} outside 0..{MAX_LEVELS}")
    if level.dtype != torch.uint8 or not level.is_cuda or not level.is_contiguous():
        raise ValueError("level must be a contiguous uint8 device tensor")
    dev, st = level.device, nat.stream()
    nch = nat.query("l3u_ccl_nchunks", n)
    parent = torch.empty(K * n, dtype=torch.int32, device=dev)
    lab = torch.empty((K, D, H, W), dtype=torch.int32, device=dev)
    cnt = torch.empty(K * (nch + 1), dtype=torch.int32, device=dev)
    offs_d = torch.empty(K + 1, dtype=torch.int32, device=dev)
    nat.call("l3u_ccl_label_lv", level.data_ptr(), k0, K, parent.data_ptr(), lab.data_ptr(),
             cnt.data_ptr(), offs_d.data_ptr(), D, H, W, st)
    offs = offs_d.cpu().numpy().astype(np.int64)
    total = int(offs[K])
    stats = np.zeros((0, 12), dtype=np.uint64)
    if total > 0:
        if prob is not None and (prob.dtype != torch.float32 or prob.numel() != n
                                 or not prob.is_contiguous()):
            raise ValueError("prob must be a contiguous float32 tensor of the level volume's size")
        sd = torch.empty(total * 12, dtype=torch.int64, device=dev)
        nat.call("l3u_ccl_stats_lv", lab.data_ptr(), nat.ptr(prob), offs_d.data_ptr(), sd.data_ptr(),
                 total, K, D, H, W, st)
        stats = sd.view(total, 12).cpu().numpy().view(np.uint64)
    comps = [Components(lab[k], int(offs[k + 1] - offs[k]), stats[int(offs[k]):int(offs[k + 1])])
             for k in range(K)]
    if target is None:
        return comps, None
    if tuple(target.labels.shape) != (D, H, W):
        raise ValueError("target labelling and level volume differ in shape")
    nt = target.num
    if total == 0 or nt == 0:
        return comps, [np.zeros((c.num + 1, nt + 1), dtype=np.int64) for c in comps]
    inter = torch.zeros(int((total + K) * (nt + 1)), dtype=torch.int32, device=dev)
    nat.call("l3u_ccl_pairs_lv", lab.data_ptr(), target.labels.data_ptr(), nt, offs_d.data_ptr(),
             inter.data_ptr(), K, n, st)
    flat = inter.cpu().numpy().astype(np.int64)
    tables = []
    for k in range(K):
        lo = int(offs[k] + k) * (nt + 1)
        tables.append(flat[lo:lo + (comps[k].num + 1) * (nt + 1)].reshape(comps[k].num + 1, nt + 1))
    return comps, tables


def _np_kind(a):
    """'f32' / 'f64' for the dtypes numpy keeps as such in `prob_map * body_mask` with a float32
    or float64 partner; None for anything whose numpy promotion is not reproduced here."""
    dt = a.dtype
    if isinstance(a, torch.Tensor):
        dt = {torch.float32: np.float32, torch.float64: np.float64, torch.bool: np.bool_,
              torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16}.get(dt)
        if dt is None:
            return None
    dt = np.dtype(dt)
    if dt == np.float64:
        return "f64"
    if dt in (np.dtype(np.float32), np.dtype(np.bool_), np.dtype(np.uint8), np.dtype(np.int8),
              np.dtype(np.int16)):
        return "f32"
    return None


def _arr(a):
    return a if isinstance(a, torch.Tensor) else np.asarray(a)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _aggregate(rows, n):
    """calculate_metrics' accumulation (metrics.py:343-404) over per-case integer rows
    (pred voxels, target voxels, overlap voxels, tp, fp, fn), in case order."""
    smooth = 1e-6
    tot_tp = tot_fp = tot_fn = 0
    inter_sum = union_sum = 0.0
    per_case = []
    for ps, ts, inter, tp, fp, fn in rows:
        inter_sum += inter
        union_sum += ps + ts
        per_case.append((2.0 * inter + smooth) / ((ps + ts) + smooth))
        tot_tp += tp
        tot_fp += fp
        tot_fn += fn
    dsc_micro = (2.0 * inter_sum + smooth) / (union_sum + smooth)
    dsc_macro = np.mean(per_case) if per_case else 0.0
    recall = tot_tp / (tot_tp + tot_fn) if (tot_tp + tot_fn) > 0 else 0.0
    precision = tot_tp / (tot_tp + tot_fp) if (tot_tp + tot_fp) > 0 else 0.0
    f1 = (2 * precision * recall) / (precision + recall) if (precision + recall) > 0 else 0.0
    return {"lesion_wise_recall": recall, "lesion_wise_precision": precision, "lesion_wise_f1": f1,
            "voxel_wise_dsc_micro": dsc_micro, "voxel_wise_dsc_macro": dsc_macro,
            "fp_per_case": tot_fp / n if n > 0 else 0.0, "tp": tot_tp, "fp": tot_fp, "fn": tot_fn,
            "dsc": dsc_micro, "recall": recall, "precision": precision}


def _sweep_case(pred, mask, tc, thr32, thr64, spacing, dev, max_workspace_bytes):
    """One case of sweep_metrics: rows[k] = (pred voxels, target voxels, overlap voxels, tp, fp,
    fn) at the k-th of the sorted distinct thresholds."""
    K = len(thr32)
    pv = _volume(pred, dev, keep_f64=True)
    mv = None
    if mask is not None:
        mv = _volume(mask, dev, keep_f64=True)
        if tuple(mv.shape) != tuple(pv.shape):
            raise ValueError("body mask and prediction differ in shape")
    tfg = (tc.labels > 0).to(torch.float32)   # target >= 0.5, as label(target, 0.5) classified it
    if pv.dtype == torch.float64 or (mv is not None and mv.dtype == torch.float64):
        # the reference compares a float64 map (or float64 product) in float64 (_foreground):
        # the levels are counted in float64 here and go through the same level kernels as the
        # "map" level with thresholds 1..K
        q = pv.double() if mv is None else pv.double() * mv.double()
        lv = torch.zeros(q.shape, dtype=torch.float32, device=dev)
        for t in thr64:
            lv += (q >= t).to(torch.float32)
        pv, mv, thr_k = lv, None, np.arange(1, K + 1, dtype=np.float32)
    else:
        thr_k = thr32
    level, hist, _ = level_map(pv, thr_k, mask=mv, target=tfg)
    n = pv.numel()
    G = max(1, min(K, nat.query("l3u_ccl_lv_max_levels", n, int(max_workspace_bytes))))
    counts = []
    for k0 in range(0, K, G):
        comps, tables = label_levels(level, min(G, K - k0), k0=k0, target=tc)
        for pc, inter in zip(comps, tables):
            counts.append(_lesion_counts(pc, tc, 0.1, 10.0, spacing, inter))
    h = hist.cpu().numpy()
    ge = np.cumsum(h[::-1], axis=0)[::-1]   # ge[l] = voxels with level >= l, per target class
    ts = int(h[:, 1].sum())
    return [(int(ge[k + 1].sum()), ts, int(ge[k + 1, 1])) + counts[k] for k in range(K)]


def sweep_metrics(predictions, labels, thresholds, spacing=(4.0, 4.0, 4.0), body_masks=None,
                  target_cache=None, case_keys=None, max_workspace_bytes=1 << 30, surface=None):
    """[calculate_metrics(predictions (* body_masks), labels, threshold=t, spacing) for t in
    thresholds], key for key and bit for bit, from ONE pass per case: one l3u_thr_levels (the
    level encoding of all distinct float32 thresholds and the voxel histogram DSC needs), one
    level-batched labelling / statistics / overlap launch each (label_levels) and one labelling of
    the target -- none when `target_cache` (a dict) holds it already under the case's key
    (`case_keys`, default the position; entries are checked against the label's shape).  The
    number of native calls per case does not depend on the number of thresholds; when the K level
    workspaces exceed `max_workspace_bytes` the levels run in groups.  Cases are numpy arrays or
    device tensors.  Inputs the level kernels do not take (a [B, D, H, W] case with B > 1, more
    than 32 distinct thresholds, dtypes numpy would promote differently) loop calculate_metrics.

    `surface` (default None: nothing changes) = {"tolerances_mm": [...], "percentile": 95.0} adds
    the boundary metrics of light_unet/surface.py to every threshold's dict: hd95_mean and
    assd_mean (means over the cases whose prediction and target surfaces are both non-empty, nan
    when there are none), nsd_mean (one value per tolerance, the mean over the cases where not
    both surfaces are empty) and surface_cases (the count the first two means ran over).  Cases
    are [D, H, W] volumes then."""
    thresholds = [t for t in thresholds]
    if surface is not None:
        from . import surface as _surface
        surf_tol, surf_q = _surface.check_config(surface)
    pred_list, label_list = _case_list(predictions, "predictions"), _case_list(labels, "labels")
    n_cases = len(pred_list)
    mask_list = [None] * n_cases if body_masks is None else _case_list(body_masks, "body_masks")
    if len(mask_list) != n_cases:
        raise ValueError("body_masks must hold one entry (or None) per case")
    if not thresholds:
        return []
    out = _sweep(pred_list, label_list, mask_list, thresholds, spacing, target_cache, case_keys,
                 max_workspace_bytes)
    if surface is not None:
        rows = [_surface.case_surface_metrics(_squeeze(_arr(p)), _squeeze(_arr(t)), thresholds, sp,
                                              surf_tol, surf_q,
                                              body_mask=None if m is None else _squeeze(_arr(m)))
                for p, t, m, sp in zip(pred_list, label_list, mask_list,
                                       _spacing_per_case(spacing, n_cases))]
        for k, d in enumerate(out):
            d.update(_surface.aggregate([r[k] for r in rows], len(surf_tol)))
    return out


def _sweep(pred_list, label_list, mask_list, thresholds, spacing, target_cache, case_keys,
           max_workspace_bytes):
    """sweep_metrics without the surface keys."""
    n_cases = len(pred_list)
    preds = [_squeeze(_arr(p)) for p in pred_list]
    targets = [_squeeze(_arr(t)) for t in label_list]
    masks = [None if m is None else _squeeze(_arr(m)) for m in mask_list]
    tf = np.asarray([float(t) for t in thresholds], dtype=np.float64)
    thr32 = np.unique(tf.astype(np.float32))
    fast = bool(np.all(np.isfinite(tf))) and len(thr32) <= MAX_LEVELS and len(label_list) == n_cases
    any64 = False
    for p, t, m in zip(preds, targets, masks):
        kinds = [_np_kind(p)] + ([] if m is None else [_np_kind(m)])
        floating = p.dtype in (torch.float32, torch.float64) if isinstance(p, torch.Tensor) \
            else p.dtype in (np.dtype(np.float32), np.dtype(np.float64))
        fast = fast and floating and None not in kinds and len(p.shape) == 3 \
            and tuple(t.shape) == tuple(p.shape) and (m is None or tuple(m.shape) == tuple(p.shape))
        any64 = any64 or "f64" in kinds
    # float64 comparisons use the thresholds as given: one float64 value per distinct float32 one
    thr64 = sorted(set(tf.tolist()))
    if any64 and len(thr64) != len(thr32):
        fast = False
    if not fast:
        host = [_host(p) if m is None else _host(p) * _host(m) for p, m in zip(pred_list, mask_list)]
        return [calculate_metrics(host, [_host(t) for t in label_list], threshold=t, spacing=spacing)
                for t in thresholds]
    spacings = _spacing_per_case(spacing, n_cases)
    dev = _device()
    keys = list(range(n_cases)) if case_keys is None else list(case_keys)
    per_case = []
    for i, (p, t, m, sp) in enumerate(zip(preds, targets, masks, spacings)):
        shape = tuple(int(v) for v in t.shape)
        hit = target_cache.get(keys[i]) if target_cache is not None else None
        if hit is not None and hit[0] == shape:
            tc = hit[1]
        else:
            tc = label(t, 0.5)
            if target_cache is not None:
                target_cache[keys[i]] = (shape, tc)
        per_case.append(_sweep_case(p, m, tc, thr32, thr64, sp, dev, max_workspace_bytes))
    out = []
    for t in thresholds:
        k = int(np.searchsorted(thr32, np.float32(t)))
        out.append(_aggregate([rows[k] for rows in per_case], n_cases))
    return out


def _case_list(x, what):
    """metrics.py:325-338: a list/tuple, or anything indexable with a leading case axis."""
    if isinstance(x, (list, tuple)):
        return list(x)
    if not (hasattr(x, "shape") and hasattr(x, "__getitem__")):
        raise TypeError(f"{what} must be a list/tuple or array-like object with shape and indexing support")
    return [x[i] for i in range(x.shape[0])]


def _spacing_per_case(spacing, n):
    """metrics.py:290-303: one (z, y, x) spacing per case; DEFAULT_SPACING when malformed."""
    default = (4.0, 4.0, 4.0)
    if n == 0:
        return []
    if isinstance(spacing, np.ndarray):
        spacing = spacing.tolist()
    if isinstance(spacing, (list, tuple)):
        if len(spacing) == 0:
            return [default] * n
        if len(spacing) == n and isinstance(spacing[0], (list, tuple, np.ndarray)):
            return [tuple(map(float, s)) for s in spacing]
        if len(spacing) == 3 and all(isinstance(s, (int, float, np.floating)) for s in spacing):
            return [tuple(map(float, spacing))] * n
    return [default] * n


def extract_bboxes(prob_map, threshold=0.3, min_volume_cc=0.5, spacing=(4.0, 4.0, 4.0),
                   expansion_voxels=0):
    """inferencer.py:62-111 (Inferencer.extract_bboxes, with config["data"]["bbox_expansion_voxels"]
    as an argument): one box per component of (prob >= threshold) with at least
    ceil(min_volume_cc / voxel cc) voxels, expanded and clipped to the volume.  expansion_voxels:
    an int, as in the reference, or one int per axis (z, y, x) for a grid that is not isotropic."""
    pm = prob_map if isinstance(prob_map, torch.Tensor) else np.asarray(prob_map)
    shape = tuple(pm.shape)
    if len(shape) != 3:
        raise ValueError(f"extract_bboxes takes a [D, H, W] probability map, got shape {shape}")
    if isinstance(expansion_voxels, (list, tuple, np.ndarray)):
        if len(expansion_voxels) != 3:
            raise ValueError("expansion_voxels takes an int or one int per axis (z, y, x), got "
                             f"{len(expansion_voxels)} values")
        ez, ey, ex = (int(v) for v in expansion_voxels)
    else:
        ez = ey = ex = expansion_voxels
    voxel_volume_cc = spacing[0] * spacing[1] * spacing[2] / 1000.0
    min_voxels = int(np.ceil(min_volume_cc / voxel_volume_cc))
    c = label(pm, threshold, min_voxels, prob=pm)
    out = []
    for cid in range(1, c.num + 1):
        s = c.stats[cid - 1]
        zmin, ymin, xmin = (int(v) for v in s[_MIN])
        zmax, ymax, xmax = (int(v) for v in s[_MAX])
        zl, zh = max(0, zmin - ez), min(shape[0] - 1, zmax + ez)
        yl, yh = max(0, ymin - ey), min(shape[1] - 1, ymax + ey)
        xl, xh = max(0, xmin - ex), min(shape[2] - 1, xmax + ex)
        conf = (c.pmax64[cid - 1] if c.pmax64 is not None
                else np.array([int(s[_PMAX])], dtype=np.uint32).view(np.float32)[0])
        out.append({"mask_id": cid,
                    "bbox_voxel": [zl, zh, yl, yh, xl, xh],
                    "bbox_mm": [float(zl * spacing[0]), float(zh * spacing[0]), float(yl * spacing[1]),
                                float(yh * spacing[1]), float(xl * spacing[2]), float(xh * spacing[2])],
                    "volume_cc": float(np.int64(s[_SIZE]) * voxel_volume_cc),
                    "confidence": float(conf)})
    return out


def min_voxels_for(min_volume_cc, spacing):
    """inferencer.py:66-68."""
    return int(math.ceil(min_volume_cc / (spacing[0] * spacing[1] * spacing[2] / 1000.0)))
