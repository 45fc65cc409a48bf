"""Generate tests/golden/tta*.npz: mirror test-time augmentation in the sliding window, computed by
the REFERENCE implementation.

Run where the reference checkout exists (never on the GPU box) with
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tta_goldens.py
It uses the reference modules make_goldens.py imports BY FILE PATH
  - <reference>/light_unet/models/unet3d.py   (Lightweight3DUNet)
  - <reference>/light_unet/utils.py           (sliding_window_inference_3d)
and writes only DATA.  The weights (`w/...`) and the two volumes come from sliding.npz and are not
stored again.

The reference has no test-time augmentation; what it computes when handed a module whose forward
is the flip mean is the contract of light_unet.utils.sliding_window_inference_3d(tta_flips=...):
    forward(x) = (F_c0(M(F_c0 x)) + F_c1(M(F_c1 x)) + ...) * float32(1 / K)
with the flip codes ascending (bit a of a code: window axis a reversed), fp32 adds in that order
starting from the code-0 term, one multiply.  The reference's own sliding_window_inference_3d
(fp32, CPU, exactly as it runs) is called with that wrapper around the reference model.

One file per case, each below the repository's 1 MiB limit for a committed file: tta.npz lists
the cases (`cases`: "<image>/<axes>" strings, `files`: the file of each) and tta_<image>_f<axes>.npz
holds `prob` (float32 [D, H, W]) and `mask_<thr>` for thr 0.1 / 0.3 / 0.5 / 0.7 as packed bits
(np.packbits of (prob >= thr).ravel()).
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_goldens   # noqa: E402  (its reference location, L3U_REFERENCE, and its by-path loads)

unet3d, rutils = make_goldens.unet3d, make_goldens.rutils

CASES = [("v40_52_48", (2,)), ("v40_52_48", (0, 1)), ("v40_52_48", (0, 1, 2)),
         ("v64_56_72", (0, 1, 2))]
THRESHOLDS = (0.1, 0.3, 0.5, 0.7)


def codes_of(axes):
    bits = sum(1 << a for a in axes)
    return [c for c in range(8) if c & ~bits == 0]


class FlipMean(torch.nn.Module):
    """forward(x) = sum over the codes of F_c(M(F_c x)), in code order, times float32(1 / K);
    x: [N, 1, pd, ph, pw], window axis a is tensor dimension 2 + a."""

    def __init__(self, model, codes):
        super().__init__()
        self.model, self.codes = model, list(codes)

    def forward(self, x):
        acc = None
        for c in self.codes:
            dims = [2 + a for a in range(3) if c >> a & 1]
            y = self.model(torch.flip(x, dims) if dims else x)
            y = torch.flip(y, dims) if dims else y
            acc = y if acc is None else acc + y
        return acc * torch.tensor(1.0 / len(self.codes), dtype=torch.float32)


def file_of(name, axes):
    return f"tta_{name}_f{''.join(str(a) for a in axes)}.npz"


def main():
    z = np.load(os.path.join(OUT, "sliding.npz"), allow_pickle=False)
    model = unet3d.Lightweight3DUNet(dropout_p=0.1)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    names, files = [], []
    for name, axes in CASES:
        wrapped = FlipMean(model, codes_of(axes))
        prob = rutils.sliding_window_inference_3d(z[f"{name}/image"], wrapped, (48, 48, 48), 0.5,
                                                  torch.device("cpu"), True).astype(np.float32)
        rec = {"prob": prob, "axes": np.array(axes, dtype=np.int64)}
        for thr in THRESHOLDS:
            rec[f"mask_{thr}"] = np.packbits((prob >= thr).ravel())
        fname = file_of(name, axes)
        np.savez_compressed(os.path.join(OUT, fname), **rec)
        size = os.path.getsize(os.path.join(OUT, fname))
        plain = z[f"{name}/prob"]
        near = max(int((np.abs(prob - t) <= 1e-4).sum()) for t in THRESHOLDS)
        print(fname, size, "bytes; max / mean change from the plain map",
              float(np.abs(prob - plain).max()), float(np.abs(prob - plain).mean()),
              "; most voxels within 1e-4 of a threshold", near, "of", prob.size)
        assert size < 1 << 20, fname
        names.append(f"{name}/{','.join(str(a) for a in axes)}")
        files.append(fname)
    np.savez_compressed(os.path.join(OUT, "tta.npz"), cases=np.array(names), files=np.array(files),
                        thresholds=np.array(THRESHOLDS))
    print("tta.npz", names)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
