"""The compute of the reference Inferencer.infer_case (inferencer.py:147-167) without its files:
sliding window -> body mask -> bounding boxes, on the device from the image to the boxes.

The reference runs every window, downloads the map, multiplies it by the body mask on the host
and uploads nothing again only because its connected components run on the host too.  Here the
mask goes into the sliding window (windows outside it are not run, utils.py `body_mask`), the
masked map stays on the device for lesion.extract_bboxes and is downloaded once, for the caller
to save.  Reading the NIfTI image / mask and writing the map and the JSON stay with the caller.
"""
import math

from . import lesion
from . import quantify as _quantify
from . import resample
from . import resegment as _resegment
from . import smooth as _smooth
from .utils import sliding_window_inference_3d


def infer_volume(image, model, config, body_mask=None, spacing=(4.0, 4.0, 4.0), threshold=None,
                 forward_cache=None, tta_flips=None, native_shape=None, uptake=None, quantify=None,
                 resegment=None, resample_order=1, smooth_fwhm_mm=None):
    """(prob_map, bboxes) of one case: prob_map the float32 numpy [D, H, W] map the reference
    saves (times `body_mask` when config["data"]["body_mask"] has both `enabled` and
    `apply_to_inference`, inferencer.py:136-137, :161-162; otherwise the mask is ignored), bboxes
    what Inferencer.extract_bboxes returns for it at `threshold` (default
    config["validation"]["default_threshold"]) with data.volume_threshold.inference_cc and
    data.bbox_expansion_voxels.  `image` and `body_mask` may be numpy arrays or device tensors
    (preprocess_volume(output="device") feeds this with no host pass); `forward_cache` as in
    sliding_window_inference_3d.  The mask's dtype is one the sliding window takes (the reference
    loads it as bool); any other raises its ValueError.  `tta_flips` (default off) is the sliding
    window's mirror test-time augmentation: None, "all" or the window axes to flip.

    `native_shape` (default None: nothing changes) is the way back for a case that was resampled
    to the network's grid (preprocess_volume(target_spacing=...)): the masked map is resampled to
    that [D, H, W] shape on the device (resample.resample_volume, order 1) and the boxes are
    extracted there, so prob_map and bbox_voxel are on the scanner's grid and `spacing` is the
    native one: the volume threshold converts through it, and the boxes grow by
    ceil(data.bbox_expansion_mm / spacing[a]) voxels on axis a (at 4 mm the reference's 3).
    `resample_order` = 3 maps the map back by cubic B-spline interpolation instead
    (resample.resample_spline with clip=(0.0, 1.0): a spline overshoots, a probability does not).

    `uptake` (default None: nothing changes, the result stays a 2-tuple) is the case's SUV volume
    on the grid the map ends on (the native grid when `native_shape` is given), numpy or device:
    the result is then (prob_map, bboxes, report) with report = quantify.lesion_uptake(uptake,
    map, ...) on the device-resident map at the boxes' threshold, minimum voxel count and spacing,
    so report["lesions"][i]["label"] == bboxes[i]["mask_id"].  `quantify` = {"peak_ml": ...,
    "dmax": ...} sets its options (quantify.check_config).  `resegment` = {"method": ..., "value":
    ..., "grow_mm": ...} (resegment.check_resegment; default None: nothing changes) has the report
    measure the lesions as resegment.resegment_lesions redraws them on the uptake: the boxes stay
    those of the network's map, and report["lesions"][k]["seed_label"] is the mask_id of the box
    the region grew from.  `smooth_fwhm_mm` (default None: nothing changes) is passed through to
    quantify.lesion_uptake: the report is that of the uptake after a Gaussian post-filter of that
    FWHM in mm, and gains "smooth"; the map and the boxes do not depend on it."""
    if resample_order not in (1, 3):
        raise ValueError("resample_order must be 1 (linear) or 3 (cubic B-spline)")
    if uptake is None and quantify is not None:
        raise ValueError("quantify sets the options of the uptake report: pass uptake too")
    if uptake is None and resegment is not None:
        raise ValueError("resegment redraws the lesions on the uptake: pass uptake too")
    if uptake is None and smooth_fwhm_mm is not None:
        raise ValueError("smooth_fwhm_mm filters the uptake: pass uptake too")
    if uptake is not None:
        peak_ml, want_dmax = _quantify.check_config(quantify)
        _resegment.check_resegment(resegment)
        if smooth_fwhm_mm is not None:
            _smooth.smooth_record(smooth_fwhm_mm, _quantify._spacing3(spacing))
        want = tuple(int(v) for v in (native_shape if native_shape is not None else image.shape[-3:]))
        if tuple(int(v) for v in uptake.shape) != want:
            raise ValueError(f"uptake must be on the grid the map ends on, {want}; got "
                             f"{tuple(uptake.shape)}")
    data = config["data"]
    bm = config.get("data", {}).get("body_mask", {})
    apply_mask = bm.get("apply_to_inference", False) and bm.get("enabled", False)
    mask = body_mask if apply_mask else None
    if threshold is None:
        threshold = config["validation"]["default_threshold"]
    device = next(model.parameters()).device
    prob = sliding_window_inference_3d(image=image, model=model,
                                       patch_size=tuple(data["patch_size"]), overlap=0.5,
                                       device=device, use_gaussian=True, output="device",
                                       forward_cache=forward_cache, body_mask=mask,
                                       tta_flips=tta_flips)
    expansion = data["bbox_expansion_voxels"]
    if native_shape is not None:
        if resample_order == 3:
            prob = resample.resample_spline(prob, native_shape, clip=(0.0, 1.0), output="device")
        else:
            prob = resample.resample_volume(prob, native_shape, order=1, output="device")
        expansion = [int(math.ceil(data["bbox_expansion_mm"] / s)) for s in spacing]
    bboxes = lesion.extract_bboxes(prob, threshold=threshold,
                                   min_volume_cc=data["volume_threshold"]["inference_cc"],
                                   spacing=spacing, expansion_voxels=expansion)
    if uptake is None:
        return prob.cpu().numpy(), bboxes   # the one download
    report = _quantify.lesion_uptake(
        uptake, prob, spacing=spacing, threshold=threshold, peak_ml=peak_ml, dmax=want_dmax,
        min_size=lesion.min_voxels_for(data["volume_threshold"]["inference_cc"], spacing),
        resegment=resegment, smooth_fwhm_mm=smooth_fwhm_mm)
    return prob.cpu().numpy(), bboxes, report
