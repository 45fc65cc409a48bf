"""Installs the MI355X hot path into an existing reference `light_unet` package.

The reference Trainer / Inferencer import the model and loss by module path
(trainer.py:16-17, inferencer.py:13) next to modules this build does not replace
(light_unet.datasets, light_unet.core.config, light_unet.models.metrics).  Both packages are
called `light_unet`, so this build is loaded under the alias `l3u_amd` (its modules only use
relative imports) and its classes are bound into the reference's module objects:

    import l3u_plugin
    l3u_plugin.install()                       # before `from light_unet.core.trainer import Trainer`
    from light_unet.core.trainer import Trainer

After install():
    light_unet.models.unet3d.Lightweight3DUNet      -> l3u_amd.models.unet3d.Lightweight3DUNet
    light_unet.models.losses.FocalTverskyLoss       -> l3u_amd.models.losses.FocalTverskyLoss
    light_unet.models.losses.get_loss_function      -> l3u_amd.models.losses.get_loss_function
    light_unet.models.losses.CombinedLoss, DiceLoss -> l3u_amd.models.losses.CombinedLoss, DiceLoss
    light_unet.models.Lightweight3DUNet / get_loss_function (package re-exports, models/__init__.py:6-8)
    light_unet.utils.sliding_window_inference_3d    -> l3u_amd.utils.sliding_window_inference_3d
Everything else in the reference package is left untouched.
"""
import importlib
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
ALIAS = "l3u_amd"

REPLACED = {
    "light_unet.utils": ("sliding_window_inference_3d",),
    "light_unet.models.unet3d": ("Lightweight3DUNet",),
    "light_unet.models.losses": ("FocalTverskyLoss", "get_loss_function", "CombinedLoss", "DiceLoss"),
    "light_unet.models": ("Lightweight3DUNet", "FocalTverskyLoss", "get_loss_function"),
}


def load():
    """This build's package, imported as `l3u_amd` (no clash with the reference's light_unet)."""
    if ALIAS in sys.modules:
        return sys.modules[ALIAS]
    pkg_dir = os.path.join(_HERE, "light_unet")
    spec = importlib.util.spec_from_file_location(
        ALIAS, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[ALIAS] = mod
    spec.loader.exec_module(mod)
    importlib.import_module(ALIAS + ".models.unet3d")
    importlib.import_module(ALIAS + ".models.losses")
    importlib.import_module(ALIAS + ".utils")
    importlib.import_module(ALIAS + ".fast_trainer")
    importlib.import_module(ALIAS + ".lesion")
    importlib.import_module(ALIAS + ".patches")
    importlib.import_module(ALIAS + ".preprocess")
    importlib.import_module(ALIAS + ".surface")
    importlib.import_module(ALIAS + ".quantify")
    importlib.import_module(ALIAS + ".inference")
    return mod


LESION = ("get_connected_components", "match_components", "calculate_lesion_metrics",
          "calculate_metrics")


def _bind_lesion(done):
    """The device lesion post-processing (light_unet/lesion.py) into the reference's metrics
    module (metrics.py:38-404) and into the modules that imported those names already
    (core.trainer: calculate_metrics; core.inferencer: get_connected_components), plus
    Inferencer.extract_bboxes (inferencer.py:62-111).  Skipped where the reference module cannot
    be imported (e.g. its scipy / sklearn / nibabel dependencies are missing)."""
    les = sys.modules[ALIAS + ".lesion"]
    try:
        metrics = importlib.import_module("light_unet.models.metrics")
    except ImportError:
        return
    names = [n for n in LESION if hasattr(metrics, n)]
    # every input form the reference functions take -- [D, H, W] volumes and batched
    # [B, D, H, W] arrays (labelled as one 4-dimensional array, as ndimage.label does) -- runs on
    # the device (csrc/lesion.hip); nothing is handed back to the host functions
    bound = {n: getattr(les, n) for n in names}
    for n in names:
        setattr(metrics, n, bound[n])
    done["light_unet.models.metrics"] = names
    for modname in ("light_unet.models", "light_unet.core.trainer", "light_unet.core.inferencer"):
        mod = sys.modules.get(modname)
        if mod is None:
            continue
        hit = [n for n in names if n in vars(mod)]
        for n in hit:
            setattr(mod, n, bound[n])
        if hit:
            done.setdefault(modname, []).extend(hit)
    inf = sys.modules.get("light_unet.core.inferencer")
    if inf is not None and hasattr(inf, "Inferencer"):
        def extract_bboxes(self, prob_map, threshold=0.3, min_volume_cc=0.5, spacing=(4.0, 4.0, 4.0)):
            return les.extract_bboxes(prob_map, threshold, min_volume_cc, spacing,
                                      self.config["data"]["bbox_expansion_voxels"])
        inf.Inferencer.extract_bboxes = extract_bboxes
        done.setdefault("light_unet.core.inferencer", []).append("Inferencer.extract_bboxes")


PREPROCESS = ("clip_and_normalize", "generate_body_mask", "calculate_voxel_thresholds")


def bind_preprocess(module):
    """The device preprocessing (light_unet/preprocess.py) into a module object the caller
    imported -- the reference's scripts/preprocess_data.py is a script, not part of its package:

        spec = importlib.util.spec_from_file_location("preprocess_data", ".../scripts/preprocess_data.py")
        pp = importlib.util.module_from_spec(spec); spec.loader.exec_module(pp)
        l3u_plugin.bind_preprocess(pp)          # preprocess_case / preprocess_dataset now call these

    Sets clip_and_normalize, generate_body_mask and calculate_voxel_thresholds (same signatures
    and results, preprocess_data.py:21-174) and returns the names it bound."""
    load()
    pre = sys.modules[ALIAS + ".preprocess"]
    for n in PREPROCESS:
        setattr(module, n, getattr(pre, n))
    return list(PREPROCESS)


DEVICE_PATCHES = (False, True, "device_draws")


def _bind_device_patches(done, draws="host"):
    """The training loaders of light_unet.datasets.loader (get_data_loader, loader.py:99-113)
    on device patches: loader._create_train_loader (loader.py:9-10, called by the standard,
    step-based and probabilistic factories) returns a DevicePatchLoader over the device twin of
    the PatchDataset / MixedPatchDataset the factory just built (its cases read once into HBM,
    its sampled locations kept; l3u_amd.patches).  Validation loaders are unchanged.
    draws="device": the loaders' per-item draws are made on the device as well."""
    loader = importlib.import_module("light_unet.datasets.loader")
    patches = sys.modules[ALIAS + ".patches"]
    ref = getattr(loader._create_train_loader, "_l3u_reference", loader._create_train_loader)

    def _create_train_loader(dataset, batch_size, shuffle=True):
        return patches.device_loader(dataset, batch_size, draws=draws)
    _create_train_loader._l3u_reference = ref
    loader._create_train_loader = _create_train_loader
    done["light_unet.datasets.loader"] = ["_create_train_loader"]


def _bind_device_locations(done):
    """PatchDataset._sample_locations (patch_dataset.py:74-100) on the device
    (l3u_amd.patches.bind_sample_locations): the case labels and body masks read as the reference
    reads them, the voxel counts and the rank-select on the device, the reference's randint calls
    on the host.  The same lists; the original stays on PatchDataset._l3u_reference_sample_locations."""
    pd = importlib.import_module("light_unet.datasets.patch_dataset")
    sys.modules[ALIAS + ".patches"].bind_sample_locations(pd.PatchDataset)
    done.setdefault("light_unet.datasets.patch_dataset", []).append("PatchDataset._sample_locations")


def install(fast_step=False, lesion=True, device_patches=False, fast_validate=False,
            device_locations=False):
    """Bind this build's model and loss into the already-importable reference package.
    Returns {module: [names]} of what was replaced.  Raises ImportError when the reference's
    light_unet.models.{unet3d,losses} cannot be imported (nothing is half-installed).

    fast_step=True also replaces Trainer.train_epoch / Trainer._train_epoch_step_based
    (trainer.py:208-347) with the graph-replayed TrainStep loops of light_unet/fast_trainer.py
    (same batches, update, TensorBoard scalars and return values; no per-step host sync; RCCL
    data parallelism when torch.distributed is initialised).  Needs light_unet.core.trainer.

    lesion=True (default) also binds the device lesion post-processing (connected components,
    matching, lesion / voxel metrics, bounding boxes: light_unet/lesion.py) where the reference's
    metrics module imports.

    device_patches=True also makes get_data_loader's training loaders cut
    and augment their patches on the device (light_unet/patches.py; num_workers = 0 draw
    semantics, DevicePatchLoader), so the graph-replayed step never waits on host workers or a
    PCIe copy.  Needs light_unet.datasets.loader (and its NIfTI reader).
    device_patches="device_draws" makes the same loaders draw on the device too (l3u_aug_draw:
    a counter-based generator seeded with the dataset's seed and the data-parallel rank), each
    full batch one hipGraph replay with no host RNG call, upload or sync: a third patch stream,
    the same distribution as the host draws but different samples; the global numpy / python
    RNGs are left alone.  Any other value raises ValueError.

    fast_validate=True also replaces Trainer.validate (trainer.py:349-445) with
    light_unet/fast_trainer.py's: probability maps stay on the device from the sliding window to
    the metrics, the captured network forward is reused across cases and epochs, and every
    threshold of threshold_sensitivity_range is evaluated from one level-batched labelling per
    case (lesion.sweep_metrics).  Same return value; the original stays reachable as
    Trainer._l3u_reference_validate.  Needs light_unet.core.trainer.  It also reads one config key
    the reference does not have, validation.tta_flips (default: absent, off): None, "all" or a
    list of window axes out of 0, 1, 2 -- the sliding window's mirror test-time augmentation
    (light_unet/utils.py `tta_flips`).  A second such key, validation.surface_metrics (default:
    absent, off) = {"tolerances_mm": [...], "percentile": 95.0}, is passed to
    lesion.sweep_metrics(surface=...): the returned metrics then carry hd95_mean, assd_mean,
    nsd_mean and surface_cases (light_unet/surface.py).

    device_locations=True also replaces PatchDataset._sample_locations (patch_dataset.py:74-100):
    every case's label and body mask are read as the reference reads them and uploaded (label as
    float64), the lesion / background voxels are counted on the device, the reference's randint
    calls are made on those counts and the drawn rows come from a rank-select on the device
    (l3u_loc_count / l3u_loc_select) instead of np.argwhere lists on the host.  The same two
    lists and the same numpy generator state; the original stays reachable as
    PatchDataset._l3u_reference_sample_locations.  Needs light_unet.datasets.patch_dataset (and
    its NIfTI reader).  Any value but True / False raises ValueError."""

    if device_locations is not True and device_locations is not False:
        raise ValueError(f"device_locations must be True or False, got {device_locations!r}")
    if isinstance(device_patches, str) and device_patches != "device_draws":
        raise ValueError(f"device_patches must be one of {DEVICE_PATCHES}, got {device_patches!r}")
    amd = load()
    trainer_mod = (importlib.import_module("light_unet.core.trainer")
                   if (fast_step or fast_validate) else None)
    src = {
        "Lightweight3DUNet": sys.modules[ALIAS + ".models.unet3d"].Lightweight3DUNet,
        "FocalTverskyLoss": sys.modules[ALIAS + ".models.losses"].FocalTverskyLoss,
        "get_loss_function": sys.modules[ALIAS + ".models.losses"].get_loss_function,
        "CombinedLoss": sys.modules[ALIAS + ".models.losses"].CombinedLoss,
        "DiceLoss": sys.modules[ALIAS + ".models.losses"].DiceLoss,
        "sliding_window_inference_3d": sys.modules[ALIAS + ".utils"].sliding_window_inference_3d,
    }
    mods = {}
    for modname in ("light_unet.utils", "light_unet.models.unet3d", "light_unet.models.losses"):
        mods[modname] = importlib.import_module(modname)
    pkg = sys.modules.get("light_unet.models")
    if pkg is not None:
        mods["light_unet.models"] = pkg
    done = {}
    for modname, mod in mods.items():
        for name in REPLACED[modname]:
            setattr(mod, name, src[name])
        done[modname] = list(REPLACED[modname])
    if fast_step:
        fast = importlib.import_module(ALIAS + ".fast_trainer")
        fast.bind(trainer_mod.Trainer)
        done["light_unet.core.trainer"] = ["Trainer.train_epoch", "Trainer._train_epoch_step_based"]
    if fast_validate:
        fast = importlib.import_module(ALIAS + ".fast_trainer")
        fast.bind_validate(trainer_mod.Trainer)
        done.setdefault("light_unet.core.trainer", []).append("Trainer.validate")
    if device_patches:
        _bind_device_patches(done, "device" if device_patches == "device_draws" else "host")
    if device_locations:
        _bind_device_locations(done)
    if lesion:
        _bind_lesion(done)
    amd.installed_into = done
    return done
