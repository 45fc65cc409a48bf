"""Whole-volume sliding-window inference on the device (drop-in for the reference's
light_unet/utils.py:11-173; imported by trainer.py:19 and inferencer.py).

Same signature, arguments, errors and result (a float32 numpy prob map [D, H, W]) as the
reference, but instead of one bs=1 forward and two host round trips per window:
  * the volume is uploaded once and windows are cut out on the device in batches
    (l3u_window_gather, zero padding past the edge as utils.py:96-113);
  * each batch runs the network forward as one replayed hipGraph (Lightweight3DUNet engine);
  * the predictions of all windows stay in HBM and one l3u_window_blend launch forms
    sum(pred * importance) / sum(importance) per voxel in the reference's window order with the
    same float32 operations (utils.py:125-135).
A model that is not this package's Lightweight3DUNet is called eagerly per batch (same device
gather / blend).  There is no CPU path: the volume is processed on `device`.
Not in the reference: `tta_flips`, mirror test-time augmentation (l3u_window_gather_flip cuts the
K flips of each window into one forward batch, l3u_window_tta_merge averages them back).
"""
import ctypes
from typing import Tuple

import numpy as np
import torch

from . import _native as nat


def _get_gaussian_importance_map(patch_size: Tuple[int, int, int]) -> np.ndarray:
    """utils.py:142-173: outer product of 1-D Gaussians (center L/2, sigma L/6), max 1, fp32."""
    def gaussian_1d(length):
        center = length / 2.0
        sigma = length / 6.0
        x = np.arange(length)
        return np.exp(-((x - center) ** 2) / (2 * sigma ** 2))

    m = np.einsum("i,j,k->ijk", gaussian_1d(patch_size[0]), gaussian_1d(patch_size[1]),
                  gaussian_1d(patch_size[2]))
    m = m / m.max()
    return m.astype(np.float32)


def window_positions(size: int, patch: int, stride: int):
    """Window starts along one axis (utils.py:64-82)."""
    pos = list(range(0, max(0, size - patch + 1), stride)) if size >= patch else []
    if size > patch and (len(pos) == 0 or pos[-1] + patch < size):
        pos.append(size - patch)
    return pos or [0]


def _gather_windows(vol, dims, pos, code, batch, patch, x):
    """`batch` windows of `vol` at `pos` into `x`; with `code` (flip codes per row, a host int
    array) each row flipped by its code."""
    D, H, W = dims
    if code is None:
        nat.call("l3u_window_gather", vol.data_ptr(), D, H, W, pos.data_ptr(), batch, *patch,
                 x.data_ptr(), nat.stream())
    else:
        nat.call("l3u_window_gather_flip", vol.data_ptr(), D, H, W, pos.data_ptr(), code, batch,
                 *patch, x.data_ptr(), nat.stream())


class _GraphForward:
    """Forward of a fixed batch of windows as one replayed graph: gather -> network."""

    def __init__(self, model, vol, D, H, W, patch, batch, device, code=None):
        self.model, self.vol, self.dims, self.patch, self.batch = model, vol, (D, H, W), patch, batch
        self.code = code   # per-row flip codes (a host int array) or None: the plain gather
        self.pos = torch.zeros(batch, 3, dtype=torch.int32, device=device)
        self.x = torch.empty(batch, 1, *patch, device=device)
        self.engine = getattr(model, "engine", None)
        self.graph = None
        if self.engine is not None:
            flat = model.flat_parameters()
            side = torch.cuda.Stream(device=device)
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side):
                self._run(flat)
            torch.cuda.current_stream(device).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = self._run(flat)

    def _gather(self):
        _gather_windows(self.vol, self.dims, self.pos, self.code, self.batch, self.patch, self.x)

    def _run(self, flat):
        self._gather()
        p, _ = self.engine.forward(flat, self.x, training=False, save=False)
        return p

    def __call__(self):
        if self.graph is not None:
            self.graph.replay()
            return self.out
        self._gather()
        return self.model(self.x)


class _CachedForward:
    """The network forward of a fixed window batch as a graph that outlives one volume
    (`forward_cache`): only the network is captured, on one static input buffer and the model's
    flat parameter buffer; the gather -- which has the volume's pointer and dimensions in its
    arguments -- runs eagerly before each replay.  Same kernels on the same values as
    _GraphForward, so the result is bitwise the same."""
    captures = 0   # graphs captured so far (tests count these)

    def __init__(self, model, patch, batch, device):
        self.model, self.patch, self.batch = model, patch, batch
        self.pos = torch.zeros(batch, 3, dtype=torch.int32, device=device)
        self.x = torch.empty(batch, 1, *patch, device=device)
        self.engine = model.engine
        self.flat = model.flat_parameters()
        self.x.zero_()
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            self.engine.forward(self.flat, self.x, training=False, save=False)
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out, _ = self.engine.forward(self.flat, self.x, training=False, save=False)
        _CachedForward.captures += 1
        self.vol = self.dims = self.code = None

    def bind(self, vol, D, H, W, code=None):
        self.vol, self.dims, self.code = vol, (D, H, W), code
        return self

    def __call__(self):
        _gather_windows(self.vol, self.dims, self.pos, self.code, self.batch, self.patch, self.x)
        self.graph.replay()
        return self.out


def _forward_for(model, vol, d, h, w, patch, B, device, forward_cache, code=None):
    """The window-batch forward: a fresh _GraphForward, or with `forward_cache` (a dict) the
    cached network graph of (model identity, window batch, patch, activation dtype).  `code`:
    the rows' flip codes (test-time augmentation); the cached graph holds no gather, so a plain
    and a flipped call of the same batch share it."""
    engine = getattr(model, "engine", None)
    if forward_cache is None or engine is None:
        return _GraphForward(model, vol, d, h, w, patch, B, device, code)
    # the engine's current activation storage, which is what _GraphForward would capture with
    key = (id(model), int(B), tuple(patch), str(engine.act_dtype))
    fwd = forward_cache.get(key)
    # the graph reads the flat parameter buffer it was captured on: a re-flattened model
    # (new storage) gets a new capture
    if fwd is None or fwd.model is not model or \
            fwd.flat.data_ptr() != model.flat_parameters().data_ptr():
        fwd = _CachedForward(model, patch, B, device)
        forward_cache[key] = fwd
    return fwd.bind(vol, d, h, w, code)


_MASK_DTYPES = "bool, uint8, int8, int16, float32"


def _checked_body_mask(body_mask, shape):
    """`body_mask` (numpy array or tensor) as a [D, H, W] float32 or uint8 array / tensor whose
    float32 value per voxel is what numpy's `prob_map * body_mask` multiplies by: bool is viewed
    as uint8, int8 / int16 are converted to float32 (exact).  ValueError for any other dtype
    (numpy would promote the product to float64) and for a shape other than `shape`.  No device
    call is made here."""
    m = body_mask
    is_t = isinstance(m, torch.Tensor)
    if not is_t:
        m = np.asarray(m)
    if len(m.shape) == 4 and m.shape[0] == 1:
        m = m[0]
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"body_mask has shape {tuple(m.shape)}, the image {tuple(shape)}")
    if is_t:
        if m.dtype == torch.bool:
            return m.contiguous().view(torch.uint8)
        if m.dtype in (torch.int8, torch.int16):
            return m.to(torch.float32)
        if m.dtype in (torch.uint8, torch.float32):
            return m
    else:
        if m.dtype == np.bool_:
            return np.ascontiguousarray(m).view(np.uint8)
        if m.dtype in (np.dtype(np.int8), np.dtype(np.int16)):
            return m.astype(np.float32)
        if m.dtype in (np.dtype(np.uint8), np.dtype(np.float32)):
            return m
    raise ValueError(f"body_mask dtype {m.dtype} is not one of {_MASK_DTYPES} (numpy would "
                     "promote prob_map * body_mask to float64: multiply such a mask on the host)")


def tta_codes(tta_flips):
    """The flip codes of mirror test-time augmentation, ascending (code 0, the identity, first):
    bit a of a code is set when window axis a (0: D, 1: H, 2: W) is reversed, and the codes are
    all those whose set bits lie within `tta_flips`.  `tta_flips`: None or () for off ([0]),
    "all" for (0, 1, 2), or a sequence of distinct axes out of {0, 1, 2}.  ValueError for anything
    else.  No device call is made here."""
    if tta_flips is None:
        return [0]
    if isinstance(tta_flips, str):
        if tta_flips != "all":
            raise ValueError(f"tta_flips must be None, 'all' or a sequence of axes, got {tta_flips!r}")
        tta_flips = (0, 1, 2)
    try:
        axes = list(tta_flips)
    except TypeError:
        raise ValueError(f"tta_flips must be None, 'all' or a sequence of axes, got {tta_flips!r}")
    bits = 0
    for a in axes:
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not 0 <= a <= 2:
            raise ValueError(f"tta_flips axes must be out of 0, 1, 2 (D, H, W), got {a!r}")
        if bits >> int(a) & 1:
            raise ValueError(f"tta_flips repeats axis {a}")
        bits |= 1 << int(a)
    return [c for c in range(8) if c & ~bits == 0]


def sliding_window_inference_3d(image: np.ndarray, model: torch.nn.Module,
                                patch_size: Tuple[int, int, int] = (48, 48, 48),
                                overlap: float = 0.5, device: torch.device = None,
                                use_gaussian: bool = True, window_batch: int = 16,
                                group=None, output: str = "numpy", forward_cache=None,
                                body_mask=None, stats=None, tta_flips=None):
    """utils.py:11-139.  `window_batch` windows run per forward (extra keyword; the result
    does not depend on it).

    `group` (extra keyword): a torch.distributed process group whose ranks (one
    per GPU, every rank calling with the same image and weights) split the window batches
    round-robin.  Each rank blends only its own windows' predictions (the others count as
    zero; the denominator sum(importance) is the full one everywhere), and one all_reduce(SUM)
    of the [D, H, W] map (RCCL over xGMI) adds the shares: the result equals the one-GPU map
    up to the order of the fp32 additions.

    `image` may also be a float32 tensor already on `device` (it is then not uploaded).
    `output="device"` returns the [D, H, W] float32 device tensor instead of copying it to the
    host.  `forward_cache` (a dict the caller keeps, e.g. across the cases and epochs of a
    validation) stores the captured network forward, so later calls with the same model, window
    batch, patch and activation dtype replay it instead of capturing again; the result is bitwise
    the uncached one.

    `body_mask` (extra keyword; a numpy array or a tensor of the image's shape, dtype bool, uint8,
    int8, int16 or float32): the result is the map times float32(body_mask), what the reference's
    callers compute right after this call (trainer.py:401-402, inferencer.py:161-162), bit for bit
    at world size 1 -- but windows without a nonzero mask voxel are not run.  l3u_window_occupancy
    marks the windows to keep, the flags are read back once, only the kept windows (in grid order,
    padded to whole batches of the same `window_batch`, so the captured forwards are the ones of a
    call without a mask) are gathered and run, and l3u_window_blend_masked blends them through a
    slot table, storing 0 where the mask is 0.  A skipped window only covers voxels the mask
    zeroes, and a voxel the mask keeps has all its windows kept, so every stored sum has the same
    terms in the same order.  With an all-zero mask no forward runs and nothing is captured.  With
    `group`, the ranks split the kept batches; voxels outside the mask are exactly 0.

    `stats` (extra keyword; a dict) is filled with `windows` (the grid), `kept` (windows run by
    all ranks together) and `forwards` (window batches this rank ran).

    `tta_flips` (extra keyword, not in the reference): mirror test-time augmentation.  None or ()
    for off, "all" for (0, 1, 2), or a sequence of distinct axes out of {0, 1, 2}: D, H and W of
    the window (anything else raises ValueError before any device call).  With k axes there are
    K = 2**k flip codes (`tta_codes`): code c has bit a set when axis a is reversed, the codes are
    all c whose set bits lie within the axes, ascending, the identity first.  For window w let x_w
    be the zero-padded pd x ph x pw window as it is cut today and F_c the reversal of the listed
    axes of that padded window (the padding moves to the low end; F_c is its own inverse).  The
    window's prediction is
        p_w = (F_c0(M(F_c0 x_w)) + F_c1(M(F_c1 x_w)) + ...) * float32(1 / K),
    summed in float32 in ascending code order as separate adds starting from the code-0 term, then
    one multiply (exact: K is a power of two).  The windows are then blended exactly as without
    it -- same kernels, order and importance map; `body_mask` and `group` work as before.  This is
    the map the plain call gives for a module whose forward is that expression.  A forward runs
    R = K * max(1, B // K) rows (B the clipped `window_batch`), the K rows of a window adjacent
    (l3u_window_gather_flip), and one l3u_window_tta_merge launch per forward writes the windows'
    means into the prediction buffer, which keeps one row per window.  When K divides B the
    forward has the plain call's batch and `forward_cache` replays the plain call's capture.
    With test-time augmentation on, `stats` also gets `tta` (= K) and `forwards` counts the
    R-row forwards; with it off the call is the one without the keyword, bit for bit."""
    if output not in ("numpy", "device"):
        raise ValueError(f"output must be 'numpy' or 'device', got {output!r}")
    codes = tta_codes(tta_flips)
    K = len(codes)
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    if len(image.shape) == 4 and image.shape[0] == 1:
        image = image[0]
    if len(image.shape) != 3:
        raise ValueError(f"Expected 3D image [D, H, W], got shape {image.shape}")
    if body_mask is not None:
        body_mask = _checked_body_mask(body_mask, image.shape)
    nat.require_device(torch.empty(0, device=device))
    d, h, w = image.shape
    pd, ph, pw = patch_size
    zs = window_positions(d, pd, max(1, int(pd * (1 - overlap))))
    ys = window_positions(h, ph, max(1, int(ph * (1 - overlap))))
    xs = window_positions(w, pw, max(1, int(pw * (1 - overlap))))
    imp = (_get_gaussian_importance_map(patch_size) if use_gaussian
           else np.ones(patch_size, dtype=np.float32))
    order = [(z, y, x) for z in zs for y in ys for x in xs]   # the reference's loop order
    nwin = len(order)
    B = max(1, min(int(window_batch), nwin))
    if K > 1:   # B windows per forward become B // K windows of K rows each
        B = max(1, B // K)
    R = K * B   # rows per forward
    P = pd * ph * pw

    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            if isinstance(image, torch.Tensor):
                vol = image.to(device=device, dtype=torch.float32).contiguous()
            else:
                vol = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(device)
            zt, yt, xt = (torch.tensor(v, dtype=torch.int32, device=device) for v in (zs, ys, xs))
            world, rank = 1, 0
            if group is not None:
                import torch.distributed as dist
                world, rank = dist.get_world_size(group), dist.get_rank(group)
            nrun, slot, mask, mcode = nwin, None, None, 0   # nrun windows run, in grid order
            if body_mask is not None:
                if isinstance(body_mask, torch.Tensor):
                    mask = body_mask.to(device).contiguous()
                else:
                    mask = torch.from_numpy(np.ascontiguousarray(body_mask)).to(device)
                mcode = 0 if mask.dtype == torch.float32 else 2   # l3u_pp_pack's dtype codes
                keep = torch.empty(nwin, dtype=torch.int32, device=device)
                nat.call("l3u_window_occupancy", mask.data_ptr(), mcode, d, h, w, zt.data_ptr(),
                         len(zs), yt.data_ptr(), len(ys), xt.data_ptr(), len(xs), pd, ph, pw,
                         keep.data_ptr(), nat.stream())
                kept = np.flatnonzero(keep.cpu().numpy())   # the one read-back
                nrun = len(kept)
            if stats is not None:
                stats.update(windows=nwin, kept=nrun,
                             forwards=len(range(rank, -(-nrun // B), world)))
                if K > 1:
                    stats["tta"] = K
            if nrun == 0:   # nothing inside the mask: no forward, no capture
                prob = torch.zeros(d, h, w, device=device)
                return prob if output == "device" else prob.cpu().numpy()
            if mask is None:
                pos_all = torch.tensor(order + [order[-1]] * ((-nwin) % B), dtype=torch.int32,
                                       device=device)
            else:
                # the kept windows' positions, padded to whole batches with the last one, and
                # the slot table (window -> row of preds, -1: not run) in one upload
                rows = np.concatenate([kept, np.repeat(kept[-1:], (-nrun) % B)])
                slot_h = np.full(nwin, -1, dtype=np.int32)
                slot_h[kept] = np.arange(nrun, dtype=np.int32)
                table = np.concatenate([np.asarray(order, dtype=np.int32)[rows].ravel(), slot_h])
                table = torch.from_numpy(table).to(device)
                pos_all, slot = table[:3 * len(rows)].view(-1, 3), table[3 * len(rows):]
            preds = (torch.zeros if world > 1 else torch.empty)(pos_all.shape[0], P, device=device)
            row_code = merge_code = None
            if K > 1:   # row g * K + j of a forward: window g under flip code j
                row_code, merge_code = (ctypes.c_int * R)(*(codes * B)), (ctypes.c_int * K)(*codes)
                pos_all = pos_all.repeat_interleave(K, dim=0)
            fwd = _forward_for(model, vol, d, h, w, (pd, ph, pw), R, device, forward_cache, row_code)
            for bi, b0 in enumerate(range(0, nrun, B)):
                if bi % world != rank:   # another rank's batch
                    continue
                fwd.pos.copy_(pos_all[b0 * K:(b0 + B) * K])
                out = fwd()
                if out.dim() != 5 or tuple(out.shape[2:]) != (pd, ph, pw):
                    raise ValueError(f"Expected 3D model output, got shape {tuple(out.shape)}")
                if K == 1:
                    preds[b0:b0 + B].copy_(out.reshape(B, P))
                else:   # the K predictions of each window, flipped back and averaged, into its row
                    rows = out.reshape(R, P).to(torch.float32).contiguous()
                    nat.call("l3u_window_tta_merge", rows.data_ptr(), merge_code, K, B, pd, ph, pw,
                             nat.ptr(preds, b0 * P), nat.stream())
            impt = torch.from_numpy(imp).to(device)
            prob = torch.empty(d, h, w, device=device)
            if mask is None:
                nat.call("l3u_window_blend", preds.data_ptr(), zt.data_ptr(), len(zs),
                         yt.data_ptr(), len(ys), xt.data_ptr(), len(xs), impt.data_ptr(), d, h, w,
                         pd, ph, pw, prob.data_ptr(), nat.stream())
            else:   # each rank's share times the mask: exact zeros outside it after the sum too
                nat.call("l3u_window_blend_masked", preds.data_ptr(), slot.data_ptr(),
                         zt.data_ptr(), len(zs), yt.data_ptr(), len(ys), xt.data_ptr(), len(xs),
                         impt.data_ptr(), mask.data_ptr(), mcode, d, h, w, pd, ph, pw,
                         prob.data_ptr(), nat.stream())
            if world > 1:
                dist.all_reduce(prob, op=dist.ReduceOp.SUM, group=group)
            return prob if output == "device" else prob.cpu().numpy()
    finally:
        model.train(was_training)
