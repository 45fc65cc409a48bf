"""l3u_plugin.install(fast_step=True, device_patches="device_draws"): get_data_loader's training
loaders draw, cut and augment their patches on the device, and Trainer.train_epoch (the fast_step
loop) runs an epoch over them in the standard and in the mixed (probabilistic) mode.

Uses the stand-in package of tests/test_device_loader_gpu.py (the reference's module layout over
.npy cases).  Checked per mode: the loader type and draw mode, the number of steps, finite
losses, that the numpy / python RNG states do not change across the epoch (the draws are the
device stream's), that the step counter advanced by one per batch, and in the mixed mode that the
Domain/* scalars the Trainer writes are the counts of the device records -- recomputed here with
patches.restate_draws over the epoch's (seed, step, batch size) sequence.  Last,
device_patches=True must still give the host-draw loader."""
import subprocess
import sys
import textwrap

import pytest

from test_device_loader_gpu import PKG, ROOT, _write_standin

pytestmark = pytest.mark.gpu

SCRIPT = '''
import importlib.util, math, random, sys
import numpy as np
import torch
sys.path[:0] = [TMP, ROOT]
spec = importlib.util.spec_from_file_location("l3u_plugin", PKG + "/l3u_plugin.py")
plug = importlib.util.module_from_spec(spec); spec.loader.exec_module(plug)
plug.load()
from light_unet.datasets import loader as L

AUG = {"gaussian_noise": {"enabled": True, "prob": 0.3, "sigma": 0.01},
       "intensity_shift": {"enabled": True, "prob": 0.5, "shift_range": [-0.1, 0.1]},
       "random_flip": {"enabled": True, "prob": 0.5, "axes": [0, 1, 2]},
       "random_rotation": {"enabled": True, "prob": 0.5, "angle_range": [-15, 15],
                           "axes": [[0, 1], [0, 2], [1, 2]]},
       "random_scale": {"enabled": True, "prob": 0.3, "scale_range": [0.9, 1.1]}}
BS = 8


def host_rng_state():
    return (np.random.get_state()[1].tobytes(), np.random.get_state()[2], random.getstate())


def loaders(mode):
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    return L.get_data_loader(TMP + "/data", TMP + "/data/train_list.txt",
                             {"augmentation": AUG, "patch_size": (32, 32, 32), "seed": 7,
                              "batch_size": BS, "mode": mode})


done = plug.install(fast_step=True, device_patches="device_draws")
assert done["light_unet.datasets.loader"] == ["_create_train_loader"]
fast = sys.modules["l3u_amd.fast_trainer"]
patches = sys.modules["l3u_amd.patches"]
Net = sys.modules["l3u_amd.models.unet3d"].Lightweight3DUNet
FTL = sys.modules["l3u_amd.models.losses"].FocalTverskyLoss


class W:
    def __init__(self):
        self.rows = {}

    def add_scalar(self, tag, value, step):
        self.rows.setdefault(tag, []).append((step, value))


class T:
    pass


t = T()
torch.manual_seed(42)
t.model = Net(encoder_channels=[8, 16, 32, 64], dropout_p=0.0).cuda()
t.criterion = FTL()
t.optimizer = torch.optim.AdamW(t.model.parameters(), lr=1e-4, weight_decay=1e-5)
t.use_step_based_mixed = False
for mode in ("standard", "probabilistic"):
    r = loaders(mode)
    lo = r["train_loader"]
    dd = lo.dataset
    assert type(lo).__name__ == "DevicePatchLoader" and dd.draws == "device", mode
    seed, step0 = dd.draw_state()   # the dataset's seed (the stand-in keeps none: the default)
    assert (seed, step0) == (42, 0), (seed, step0)
    t.writer = W()
    t.train_loader = lo
    t.use_mixed_training = mode == "probabilistic"
    t.train_dataset = r.get("train_dataset")
    before = host_rng_state()
    avg = fast.train_epoch(t, 0)
    assert host_rng_state() == before, mode
    n = len(dd)
    sizes = [min(BS, n - b0) for b0 in range(0, n, BS)]
    steps = t.writer.rows["Loss/train_step"]
    assert len(steps) == len(lo) == len(sizes) >= 3 and sizes[-1] != BS, (mode, sizes)
    assert all(math.isfinite(v) for _, v in steps) and math.isfinite(avg), (mode, steps)
    assert dd.draw_state() == (seed, len(sizes)), (mode, dd.draw_state())
    if mode == "probabilistic":
        specs = [dd.fl.draw_spec(), dd.dlbcl.draw_spec()]
        recs = [x for s, b in enumerate(sizes) for x in patches.restate_draws(seed, s, b, specs, dd.fl_ratio)]
        fl = sum(x.domain == 0 for x in recs)
        assert 0 < fl < n
        rows = t.writer.rows
        assert rows["Domain/fl_samples"] == [(0, fl)], (rows["Domain/fl_samples"], fl)
        assert rows["Domain/dlbcl_samples"] == [(0, n - fl)]
        assert r["train_dataset"].get_sample_counts() == {
            "fl_samples": fl, "dlbcl_samples": n - fl, "total_samples": n}
    print("EPOCH OK", mode, len(sizes), avg)

# device_patches=True keeps its meaning: the host-draw loader
plug.install(fast_step=True, device_patches=True)
r = loaders("standard")
lo = r["train_loader"]
assert type(lo).__name__ == "DevicePatchLoader" and lo.dataset.draws == "host"
before = host_rng_state()
x, _ = next(iter(lo))
assert x.shape == (BS, 1, 32, 32, 32) and host_rng_state() != before
print("HOST OK")
'''


def test_trainer_epoch_on_device_draws(cuda, tmp_path):
    _write_standin(tmp_path)
    script = f"TMP, ROOT, PKG = {str(tmp_path)!r}, {ROOT!r}, {PKG!r}\n" + textwrap.dedent(SCRIPT)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.count("EPOCH OK") == 2 and "HOST OK" in r.stdout, r.stdout
