"""The reference Trainer's training loops on the graph-replayed TrainStep.

`l3u_plugin.install(fast_step=True)` binds `train_epoch` and `train_epoch_step_based` below onto
the reference `light_unet.core.trainer.Trainer` (as `train_epoch` / `_train_epoch_step_based`,
trainer.py:208-258 / :260-347).  They keep the reference loops' meaning:

  * the same batches in the same order (the reference DataLoaders are iterated unchanged; the
    step-based mode runs every FL batch, then round(fl_batches * dlbcl_steps_ratio) DLBCL steps
    (or `dlbcl_steps`), re-iterating the DLBCL loader when it runs out, trainer.py:262-269,
    :301-312);
  * the same update: forward -> criterion -> backward -> AdamW(lr, weight_decay, betas, eps of
    the Trainer's torch optimizer), with the learning rate read from that optimizer at the start
    of every epoch, so the Trainer's CosineAnnealingLR / ReduceLROnPlateau steps (trainer.py:
    532-542) drive it;
  * the same TensorBoard scalars at the same global steps (Loss/train_step, Loss/fl_step,
    Loss/dlbcl_step, Domain/*, Loss/fl_avg|dlbcl_avg|combined) and the same return value.

What changes is how a step runs: each batch is copied into the static input buffers of a
hipGraph-captured TrainStep and the graph is replayed (forward, loss, backward and the update
in one replay; with torch.distributed initialised, the FocalTversky sums and the flat gradient
are all-reduced over RCCL between the graph segments, exchange.py).  Per-step losses stay on the
device and are read ONCE per epoch (the reference syncs on loss.item() every step,
trainer.py:234, :293, :323).  A batch whose shape differs from the captured one (a ragged last
batch) runs the same step eagerly.

The torch optimizer is not stepped; its per-parameter state is kept as views of the flat AdamW
state (exp_avg / exp_avg_sq, and `step`), refreshed at the end of every epoch, so
`optimizer.state_dict()` in the Trainer's checkpoints (trainer.py:447-470) holds the real
moments.  The criterion may be FocalTverskyLoss, CombinedLoss (`use_combined_loss`) or DiceLoss
(exact types, no reduce_hook): all three run inside the out_conv launches of the step.  Any
other criterion falls back to the reference loop.

`l3u_plugin.install(fast_validate=True)` binds `validate` below as `Trainer.validate`
(trainer.py:349-445): the same cases, masks, spacings, thresholds, `_is_better_metric` calls and
return value, but the probability maps stay on the device from the sliding window to the metrics
(`sliding_window_inference_3d(output="device", forward_cache=...)`), and all thresholds of
`threshold_sensitivity_range` are evaluated by one `lesion.sweep_metrics` call: one level
encoding and one level-batched labelling per case instead of an upload and two labellings per
case and threshold.  The captured network forward and the targets' labellings are kept per
Trainer, so later epochs neither capture nor label the targets again.  A body mask whose product
with the map numpy keeps in float32 goes into the sliding window (`body_mask=`): windows outside
it are not run and the map arrives already multiplied by it.  One config key the reference does
not have, `validation.tta_flips` (absent: off), turns on the sliding window's mirror test-time
augmentation; another, `validation.surface_metrics` (absent: off), adds the boundary metrics of
`light_unet/surface.py` to the returned dict (`lesion.sweep_metrics(surface=...)`).
"""
import torch

from . import lesion
from .models.losses import CombinedLoss, DiceLoss, FocalTverskyLoss
from .train_step import TrainStep
from .utils import sliding_window_inference_3d

_FALLBACK = "_l3u_reference_loops"
_FALLBACK_VALIDATE = "_l3u_reference_validate"


class FastLoop:
    """Per-Trainer state: one TrainStep on the model's flat buffers, its captured graph, and the
    device-side loss history of the running epoch."""

    def __init__(self, trainer, group=None, ftl_mode="exact"):
        model, opt = trainer.model, trainer.optimizer
        crit = trainer.criterion
        pg = opt.param_groups[0]
        # the criterion itself: FocalTversky keeps its entry points, CombinedLoss / DiceLoss run
        # as the loss family in the same launches (train_step.parse_loss)
        self.step = TrainStep(model, crit, lr=pg["lr"], weight_decay=pg["weight_decay"],
                              betas=pg["betas"], eps=pg["eps"], group=group, ftl_mode=ftl_mode)
        if self.step.world > 1:   # identical initial weights on every rank (DDP semantics)
            import torch.distributed as dist
            dist.broadcast(self.step.flat, 0, group=group)
        self._load_torch_state(opt)
        self.shape = None
        self.xs = self.ts = None
        self.hist = None
        self.n = 0

    # ------------------------------------------------------------ optimizer state mirroring
    def _params(self, opt):
        return [p for g in opt.param_groups for p in g["params"]]

    def _load_torch_state(self, opt):
        """Continue from the torch optimizer's moments if it has any (e.g. a resumed run)."""
        st, model = self.step.opt, self.step.model
        slices = dict(zip([id(p) for p in model.parameters()], model._slices))
        steps = set()
        for p in self._params(opt):
            s = opt.state.get(p)
            if not s or "exp_avg" not in s:
                continue
            off, n, _ = slices[id(p)]
            st.m[off:off + n].copy_(s["exp_avg"].reshape(-1))
            st.v[off:off + n].copy_(s["exp_avg_sq"].reshape(-1))
            steps.add(int(float(s["step"])))
        if len(steps) > 1:
            raise ValueError(f"parameters of the torch optimizer are at different steps {steps}")
        if steps:
            st.step_t.fill_(steps.pop())

    def export_torch_state(self, opt):
        """Make opt.state the flat AdamW state (views; `step` as torch.optim.AdamW stores it)."""
        st, model = self.step.opt, self.step.model
        t = float(st.step_t.item())
        slices = dict(zip([id(p) for p in model.parameters()], model._slices))
        for p in self._params(opt):
            off, n, shape = slices[id(p)]
            opt.state[p] = {"step": torch.tensor(t, dtype=torch.float32),
                            "exp_avg": st.m[off:off + n].view(shape),
                            "exp_avg_sq": st.v[off:off + n].view(shape)}

    # ------------------------------------------------------------ steps
    def begin_epoch(self, lr, n_steps):
        self.step.opt.set_lr(lr)
        dev = self.step.flat.device
        self.hist = torch.zeros(max(int(n_steps), 1), dtype=torch.float32, device=dev)
        self.n = 0

    def run(self, images, labels):
        """One training step on a host (or device) batch; the loss stays on the device."""
        dev = self.step.flat.device
        x = images.float()
        t = labels.float()
        if tuple(x.shape) != tuple(t.shape):
            raise ValueError(f"images {tuple(x.shape)} and labels {tuple(t.shape)} differ")
        if self.shape is None:
            self.shape = tuple(x.shape)
            self.xs = torch.empty(self.shape, dtype=torch.float32, device=dev)
            self.ts = torch.empty(self.shape, dtype=torch.float32, device=dev)
            self.xs.copy_(x)
            self.ts.copy_(t)
            self.step.capture(self.xs, self.ts)   # side-effect free (TrainStep.capture)
        if tuple(x.shape) == self.shape:
            self.xs.copy_(x, non_blocking=True)
            self.ts.copy_(t, non_blocking=True)
            loss = self.step.replay()
        else:
            loss = self.step(x.to(dev).contiguous(), t.to(dev).contiguous())
        if self.n >= self.hist.numel():   # more steps than announced: grow (rare)
            self.hist = torch.cat([self.hist, torch.zeros_like(self.hist)])
        self.hist[self.n:self.n + 1].copy_(loss.reshape(1))
        self.n += 1

    def losses(self):
        """The epoch's per-step losses (one device->host copy)."""
        return self.hist[:self.n].double().cpu().tolist()


def _loop(self):
    fl = getattr(self, "_l3u_fast", None)
    if fl is None:
        fl = FastLoop(self, ftl_mode=getattr(self, "l3u_ftl_mode", "exact"))
        self._l3u_fast = fl
    return fl


def _usable(self):
    return type(self.criterion) in (FocalTverskyLoss, CombinedLoss, DiceLoss) and \
        getattr(self.criterion, "reduce_hook", None) is None


def _tqdm(it, **kw):
    try:
        from tqdm import tqdm
        return tqdm(it, **kw)
    except ImportError:
        return it


def train_epoch(self, epoch):
    """Trainer.train_epoch (trainer.py:208-258) on the graph-replayed step."""
    self.model.train()
    if self.use_step_based_mixed:
        return self._train_epoch_step_based(epoch)
    if not _usable(self):
        return getattr(type(self), _FALLBACK)["train_epoch"](self, epoch)
    if self.use_mixed_training and self.train_dataset is not None:
        self.train_dataset.reset_sample_counts()
    fl = _loop(self)
    nb = len(self.train_loader)
    fl.begin_epoch(self.optimizer.param_groups[0]["lr"], nb)
    for images, labels in _tqdm(self.train_loader, desc=f"Epoch {epoch+1} [Train]"):
        fl.run(images, labels)
    losses = fl.losses()
    fl.export_torch_state(self.optimizer)
    for i, v in enumerate(losses):
        self.writer.add_scalar("Loss/train_step", v, epoch * nb + i)
    avg = sum(losses) / len(losses)
    if self.use_mixed_training and self.train_dataset is not None:
        c = self.train_dataset.get_sample_counts()
        if c["total_samples"] > 0:
            self.writer.add_scalar("Domain/fl_samples", c["fl_samples"], epoch)
            self.writer.add_scalar("Domain/dlbcl_samples", c["dlbcl_samples"], epoch)
            self.writer.add_scalar("Domain/fl_ratio", c["fl_samples"] / c["total_samples"], epoch)
            self.writer.add_scalar("Domain/dlbcl_ratio", c["dlbcl_samples"] / c["total_samples"],
                                   epoch)
    return avg


def dlbcl_step_count(config, fl_batches):
    """trainer.py:262-269: the explicit `dlbcl_steps`, else round(fl_batches * ratio)."""
    mixed = config.get("training", {}).get("mixed_domains", {})
    override = mixed.get("dlbcl_steps", None)
    if override is not None:
        return int(override)
    return round(fl_batches * mixed.get("dlbcl_steps_ratio", 0.0))


def train_epoch_step_based(self, epoch):
    """Trainer._train_epoch_step_based (trainer.py:260-347) on the graph-replayed step."""
    if not _usable(self):
        return getattr(type(self), _FALLBACK)["_train_epoch_step_based"](self, epoch)
    fl_batches = len(self.fl_loader)
    dlbcl_steps = dlbcl_step_count(self.config, fl_batches)
    base = epoch * (fl_batches + dlbcl_steps)
    fl = _loop(self)
    fl.begin_epoch(self.optimizer.param_groups[0]["lr"], fl_batches + max(dlbcl_steps, 0))
    for images, labels in _tqdm(self.fl_loader, desc=f"Epoch {epoch+1} [FL]", position=0):
        fl.run(images, labels)
    fl_steps = fl.n
    if dlbcl_steps > 0:
        it = iter(self.dlbcl_loader)
        for _ in _tqdm(range(dlbcl_steps), desc=f"Epoch {epoch+1} [DLBCL]", position=0):
            try:
                images, labels = next(it)
            except StopIteration:        # re-iterate the DLBCL loader (trainer.py:307-312)
                it = iter(self.dlbcl_loader)
                images, labels = next(it)
            fl.run(images, labels)
    losses = fl.losses()
    fl.export_torch_state(self.optimizer)
    fl_l, dl_l = losses[:fl_steps], losses[fl_steps:]
    for i, v in enumerate(fl_l):
        self.writer.add_scalar("Loss/train_step", v, base + i)
        self.writer.add_scalar("Loss/fl_step", v, base + i)
    for i, v in enumerate(dl_l):
        self.writer.add_scalar("Loss/train_step", v, base + fl_steps + i)
        self.writer.add_scalar("Loss/dlbcl_step", v, base + fl_steps + i)
    total = len(losses)
    fl_avg = sum(fl_l) / len(fl_l) if fl_l else 0.0
    dl_avg = sum(dl_l) / len(dl_l) if dl_l else 0.0
    combined = sum(losses) / total if total else 0.0
    self.writer.add_scalar("Domain/fl_steps", len(fl_l), epoch)
    self.writer.add_scalar("Domain/dlbcl_steps", len(dl_l), epoch)
    self.writer.add_scalar("Domain/fl_ratio", len(fl_l) / total if total else 0.0, epoch)
    self.writer.add_scalar("Domain/dlbcl_ratio", len(dl_l) / total if total else 0.0, epoch)
    self.writer.add_scalar("Loss/fl_avg", fl_avg, epoch)
    self.writer.add_scalar("Loss/dlbcl_avg", dl_avg, epoch)
    self.writer.add_scalar("Loss/combined", combined, epoch)
    return combined


def bind(trainer_cls):
    """Replace the two loops on the Trainer class (keeping the originals for the fallback)."""
    if _FALLBACK not in trainer_cls.__dict__:
        setattr(trainer_cls, _FALLBACK, {"train_epoch": trainer_cls.train_epoch,
                                         "_train_epoch_step_based":
                                             trainer_cls._train_epoch_step_based})
    trainer_cls.train_epoch = train_epoch
    trainer_cls._train_epoch_step_based = train_epoch_step_based
    return trainer_cls


# ---------------------------------------------------------------------- validation
def evaluate_maps(prob_maps, labels, spacings, thresholds, tie_threshold, is_better,
                  body_masks=None, target_cache=None, case_keys=None, surface=None):
    """The post-inference stage of Trainer.validate (trainer.py:423-445) on probability maps
    (numpy or device): the metrics at every threshold from one lesion.sweep_metrics call, then the
    reference's selection loop with `is_better` (the Trainer's _is_better_metric).  Returns the
    chosen metrics dict with best_threshold / best_recall / best_dsc_macro.  `surface` (None: off)
    is sweep_metrics' argument of that name: the chosen dict then carries the boundary metrics."""
    thresholds = list(thresholds)
    kw = {} if surface is None else {"surface": surface}
    swept = lesion.sweep_metrics(prob_maps, labels, thresholds, spacing=spacings,
                                 body_masks=body_masks, target_cache=target_cache,
                                 case_keys=case_keys, **kw)
    best_threshold, best_metrics = thresholds[0], swept[0]
    best_recall = best_metrics["lesion_wise_recall"]
    best_dsc_macro = best_metrics["voxel_wise_dsc_macro"]
    for threshold, metrics in zip(thresholds[1:], swept[1:]):
        better, _ = is_better(metrics["lesion_wise_recall"], metrics["voxel_wise_dsc_macro"],
                              best_recall, best_dsc_macro, tie_threshold)
        if better:
            best_recall = metrics["lesion_wise_recall"]
            best_dsc_macro = metrics["voxel_wise_dsc_macro"]
            best_threshold = threshold
            best_metrics = metrics
    best_metrics["best_threshold"] = best_threshold
    best_metrics["best_recall"] = best_recall
    best_metrics["best_dsc_macro"] = best_dsc_macro
    return best_metrics


def _case_id(case_ids, b):
    """The batch's b-th case id as a hashable key, or None where the loader gives none."""
    try:
        cid = case_ids[b]
    except (TypeError, IndexError, KeyError):
        return None
    if isinstance(cid, torch.Tensor):
        cid = cid.tolist()
    if isinstance(cid, list):
        cid = tuple(cid)
    try:
        hash(cid)
    except TypeError:
        return None
    return cid


def validate(self, epoch):
    """Trainer.validate (trainer.py:349-445) with device-resident probability maps."""
    self.model.eval()
    state = getattr(self, "_l3u_validate", None)
    if state is None:
        state = self._l3u_validate = {"forward": {}, "targets": {}}
    maps, all_labels, all_spacings, masks, keys = [], [], [], [], []
    target_spacing = self._get_target_spacing()
    default_threshold = self.config["validation"]["default_threshold"]
    patch_size = tuple(self.config["data"]["patch_size"])
    bm = self.config.get("data", {}).get("body_mask", {})
    apply_body_mask = bm.get("apply_to_validation", False) and bm.get("enabled", False)
    # mirror test-time augmentation: a key the reference configs do not have (absent: off)
    tta_flips = self.config["validation"].get("tta_flips")
    # boundary metrics (light_unet/surface.py): another key of this build's own (absent: off)
    surface_metrics = self.config["validation"].get("surface_metrics")
    dev = torch.device(self.device)
    with torch.no_grad():
        for batch in _tqdm(self.val_loader, desc=f"Epoch {epoch+1} [Val]"):
            case_ids = spacings = body_masks = None
            if isinstance(batch, (list, tuple)) and len(batch) >= 5:
                images, labels, case_ids, spacings, body_masks = batch[:5]
            elif isinstance(batch, (list, tuple)) and len(batch) >= 4:
                images, labels, case_ids, spacings = batch[:4]
            else:
                images, labels = batch[0], batch[1]
            if images.ndim not in (4, 5):
                raise ValueError(f"Unexpected image shape: {images.shape}")
            for b in range(images.shape[0]):
                pick = (lambda t: t[b, 0]) if images.ndim == 5 else (lambda t: t[b])
                image = pick(images).to(device=dev, dtype=torch.float32)
                mask = pick(body_masks) if (apply_body_mask and body_masks is not None) else None
                # a mask whose product with the map numpy keeps in float32 goes into the sliding
                # window: windows outside it are not run and the map comes back multiplied by it
                # (the float32 product the metrics would form), so the metrics get no mask
                kw = {} if tta_flips is None else {"tta_flips": tta_flips}
                if mask is not None and lesion._np_kind(mask) == "f32" \
                        and tuple(mask.shape) == tuple(image.shape):
                    kw["body_mask"], mask = mask, None
                prob = sliding_window_inference_3d(image=image, model=self.model,
                                                   patch_size=patch_size, overlap=0.5, device=dev,
                                                   use_gaussian=True, output="device",
                                                   forward_cache=state["forward"], **kw)
                # numpy's prob_map * body_mask with the mask's own dtype (a host tensor becomes the
                # numpy array the reference multiplies by)
                masks.append(mask.cpu().numpy() if isinstance(mask, torch.Tensor) and not mask.is_cuda
                             else mask)
                maps.append(prob)
                all_labels.append(pick(labels).cpu().numpy())
                all_spacings.append(self._resolve_spacing_value(spacings, b, target_spacing)
                                    if spacings is not None else target_spacing)
                cid = _case_id(case_ids, b) if case_ids is not None else None
                keys.append(("pos", len(keys)) if cid is None else ("id", cid))
    if len(maps) == 0:
        return 0.0, {"lesion_wise_recall": 0.0, "lesion_wise_precision": 0.0,
                     "voxel_wise_dsc_macro": 0.0, "voxel_wise_dsc_micro": 0.0,
                     "fp_per_case": 0.0, "best_threshold": default_threshold,
                     "best_recall": 0.0, "best_dsc_macro": 0.0}
    if len(set(keys)) != len(keys):   # repeated ids: positions are the only safe keys
        keys = [("pos", i) for i in range(len(keys))]
    thresholds = self.config["validation"].get("threshold_sensitivity_range", [default_threshold])
    tie_threshold = self.config["metrics"]["model_selection"].get("tie_threshold", 0.0)
    best = evaluate_maps(maps, all_labels, all_spacings, thresholds, tie_threshold,
                         self._is_better_metric,
                         body_masks=masks if any(m is not None for m in masks) else None,
                         target_cache=state["targets"], case_keys=keys, surface=surface_metrics)
    return 0.0, best


def bind_validate(trainer_cls):
    """Replace Trainer.validate (the original stays reachable as _l3u_reference_validate)."""
    if _FALLBACK_VALIDATE not in trainer_cls.__dict__:
        setattr(trainer_cls, _FALLBACK_VALIDATE, trainer_cls.validate)
    trainer_cls.validate = validate
    return trainer_cls
