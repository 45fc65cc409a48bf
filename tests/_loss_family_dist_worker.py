"""Worker of tests/test_loss_family_gpu.py::test_trainstep_combined_two_ranks (not a test module).

Every rank runs the product TrainStep with the reference's `use_combined_loss` config on its half
of a bs-4 batch at 16^3:
  A  exact mode, dropout 0: one eager step (loss, flat gradient after the exchange);
  B  local mode, dropout 0: one eager step (the averaged flat gradient).
Rank r saves its arrays to <out>/rank<r>.npz.  Launched by torch.distributed.run (gloo, both ranks
on cuda:0), a fresh child process per rank.  argv: <out>."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "light-3d-unet-front_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SIZE = 16
LOSS_CFG = {"name": "FocalTverskyLoss", "alpha": 0.7, "beta": 0.3, "gamma": 0.75,
            "use_combined_loss": True, "combined_loss_weights": {"focal_tversky": 0.8, "bce": 0.2}}


def batch(size=SIZE):
    """The global bs-4 batch every process draws identically (seeded)."""
    rng = np.random.default_rng(11)
    x = rng.random((4, 1, size, size, size), dtype=np.float32)
    t = (rng.random((4, 1, size, size, size)) > 0.95).astype(np.float32)
    return x, t


def fresh_model(dev):
    from light_unet.models.unet3d import Lightweight3DUNet
    torch.manual_seed(42)
    return Lightweight3DUNet(dropout_p=0.0).to(dev).train()


def main():
    out = sys.argv[1]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    from light_unet.train_step import TrainStep
    per = 4 // world
    sl = slice(rank * per, (rank + 1) * per)
    x, t = batch()
    dx = torch.from_numpy(x[sl].copy()).to(dev)
    dt = torch.from_numpy(t[sl].copy()).to(dev)
    res = {}
    ts = TrainStep(fresh_model(dev), LOSS_CFG, ftl_mode="exact")
    loss = ts(dx, dt)
    torch.cuda.synchronize()
    res["A_loss1"] = np.float64(loss.item())
    res["A_g1"] = ts.gflat.cpu().numpy().copy()
    ts = TrainStep(fresh_model(dev), LOSS_CFG, ftl_mode="local")
    ts(dx, dt)
    torch.cuda.synchronize()
    res["B_g1"] = ts.gflat.cpu().numpy().copy()
    np.savez(os.path.join(out, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
