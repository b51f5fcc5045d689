"""The layout of the tail wrappers (hyperpri_amd/_args.py, losses.py, metrics.py, optim.py, trainer.py): every name that was importable
from trainer, components, evaluate and distance before trainer.py was split still is, and is the object of its new home; the
placement errors keep their texts; the step-row buffer grows as it did; the fp32 helper allocates nothing for fp32.  No GPU, no
library: nothing here launches."""
import importlib

import pytest
import torch

# dir() of the four modules before the split (typing names and imported third-party modules left out), by the module each name
# lives in now.  None: it stayed where it was.
NAMES = {
    "trainer": {
        None: ["SegmentationModel", "forward_loss", "load_checkpoint", "network_state_dict", "_lib"],
        "losses": ["BCEWithLogitsLoss", "CrossEntropyLoss", "DiceBCELoss", "DiceLoss", "FocalLoss", "MAX_SKELETON_ITERS", "SegLoss", "TverskyLoss",
                   "_BCEFn", "_CEFn", "_FusedLossFn", "_SegLossFn", "_SoftSkeletonFn", "_check_iters", "_clDiceFn", "_takes_fused_head",
                   "clDiceLoss", "soft_skeleton"],
        "metrics": ["PRCurve", "SegConfusion", "SegCounts", "_StepConfusion", "_StepCounts", "_confusion_pass", "_split_counts", "argmax_classes",
                    "average_precision", "best_dice_threshold", "metrics_from_counts", "multiclass_metrics_from_confusion"],
        "optim": ["FusedAdam", "FusedSGD", "_ptr_array"],
        "_args": ["MAX_CLASSES", "_TARGET_KIND", "_class_logits", "_class_target", "_flat", "_ignore_args", "_planes", "_require_cuda", "_scalar"],
    },
    "components": {
        None: ["STAT_NAMES", "TILE_H", "TILE_W", "_TRUTH_KIND", "_check_clean_args", "_check_connectivity", "_clean_launch", "_label_image",
               "_label_truth", "_lib", "_workspace", "clean_mask", "clean_reference", "component_table", "components_reference",
               "label_components", "stats_dict", "table_reference"],
        "_args": ["_as_images", "_decision_input", "_map3d", "_p", "_require_cuda", "_require_device", "_stream"],
    },
    "evaluate": {
        None: ["ALPHA", "CLEAN_LOGIT", "HSI_BANDS", "HSI_GAMMA", "PALETTE", "RGB_BANDS", "RGB_GAMMA", "SplitPrediction", "_CLASS_COLOURS",
               "_at_threshold", "_bce", "_lib", "_mean_defined", "_names", "_require_device", "_size_groups", "_view_logits", "_write_picture",
               "centerline_metrics", "clean_prediction", "color_classmaps", "color_segmaps", "default_class_palette", "evaluate_multiclass",
               "object_metrics", "patch_last_point", "predict_split", "root_traits", "surface_metrics", "test_net", "tta_merge", "validate_net",
               "write_segmaps", "write_spreadmaps"],
        "tta": ["TTA", "VIEW_CODES", "apply_view", "view_shape"],
        "metrics": ["PRCurve", "SegCounts", "_confusion_pass", "_split_counts", "average_precision", "best_dice_threshold",
                    "multiclass_metrics_from_confusion"],
        "_args": ["MAX_CLASSES", "_TARGET_KIND", "_class_logits", "_class_target", "_ignore_args", "_image4d", "_p", "_require_cuda", "_stream"],
    },
    "distance": {
        None: ["COL_THREADS", "HIST_LDS_BINS", "ROWS_PER_GROUP", "ROW_THREADS", "SITES", "THIN_CHECK_PAIRS", "TOLERANCES", "TRAIT_NAMES", "_SK_PLUS",
               "_SK_WINDOW", "_check_edt_shape", "_check_sites", "_decide", "_edt_image", "_edt_launch", "_lib", "_sites_reference", "_sk_route",
               "_sk_stack", "_thin", "_thin_pass", "_traits", "_truth_input", "_value_at_rank", "boundary_reference", "centerline_counts",
               "centerline_from_counts", "centerline_metrics", "distance_transform", "edt_max_width", "edt_reference", "links_reference",
               "root_traits", "select_hist", "skeleton_links", "skeletonize", "soft_skeleton_reference", "surface_distances",
               "surface_hist_reference", "surface_metrics_from_hist", "thin_reference", "traits_from_counts", "traits_reference"],
        "_args": ["_as_images", "_decision_input", "_map3d", "_p", "_require_device", "_stream"],
    },
}


def _module(name):
    return importlib.import_module("hyperpri_amd." + name)


@pytest.mark.parametrize("old", sorted(NAMES))
def test_every_name_is_still_importable_from_where_it_was(old):
    was = _module(old)
    for home, names in NAMES[old].items():
        for name in names:
            assert hasattr(was, name), f"{old}.{name} is gone"
            if home is not None:
                assert getattr(was, name) is getattr(_module(home), name), f"{old}.{name} is not {home}.{name}"


def test_the_engine_helpers_are_the_engines_own():
    from hyperpri_amd import _args, engine
    for name in ("_p", "_stream", "_rup", "_require_cuda"):
        assert getattr(_args, name) is getattr(engine, name)


# The three wordings of "this tensor is not on the device", as they read before they were folded into one function
HOT = "hyperpri_amd: %s is on cpu; the hot path exists only as HIP kernels for MI355X (no CPU fallback). Move the module and its inputs to a ROCm device."
MAPS = "hyperpri_amd: %s is on cpu; connected components exist only as HIP kernels for MI355X (no CPU fallback). Move the tensors to a ROCm device."
EVAL = "hyperpri_amd: %s is on cpu; evaluation exists only as HIP kernels for MI355X (no CPU fallback). Move the batches to a ROCm device."


class _OnDevice:
    """Stands in for contiguous fp32 (1, K, 4, 4) logits on a device, as far as ``_class_logits`` and the ``update`` methods look."""
    is_cuda, dtype, device = True, torch.float32, -1        # (torch.cuda.device(-1) is a no-op)

    def __init__(self, K: int = 3):
        self.shape = (1, K, 4, 4)

    def detach(self):
        return self

    def dim(self):
        return 4

    def is_contiguous(self):
        return True


def _message(call) -> str:
    with pytest.raises(RuntimeError) as e:
        call()
    return str(e.value)


def test_placement_errors_keep_their_texts():
    import hyperpri_amd as H
    from hyperpri_amd import distance as D
    from hyperpri_amd import evaluate as E
    x, m, u8 = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(2, 4, 5, dtype=torch.uint8)
    logits, classes = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    split = H.SplitPrediction(torch.zeros(40), torch.zeros(40), [0, 20, 40], [(4, 5), (4, 5)], ["a", "b"])
    assert _message(lambda: H.SegCounts().update(x, m)) == HOT % "prediction"
    assert _message(lambda: H.PRCurve().update(x, m)) == HOT % "prediction"
    assert _message(lambda: H.average_precision(x, m)) == HOT % "prediction"
    assert _message(lambda: H.BCEWithLogitsLoss()(x, m)) == HOT % "BCEWithLogitsLoss input"
    assert _message(lambda: H.DiceLoss()(x, m)) == HOT % "SegLoss input"
    assert _message(lambda: H.clDiceLoss(alpha=1.0)(x, m)) == HOT % "clDiceLoss input"
    assert _message(lambda: H.soft_skeleton(x, 2)) == HOT % "soft_skeleton input"
    assert _message(lambda: H.forward_loss(torch.nn.Identity(), x, m)) == HOT % "input tensor"
    assert _message(lambda: H.CrossEntropyLoss()(logits, classes)) == HOT % "CrossEntropyLoss input"
    assert _message(lambda: H.argmax_classes(logits)) == HOT % "argmax_classes input"
    assert _message(lambda: H.SegConfusion(3).update(logits, classes)) == HOT % "SegConfusion prediction"
    assert _message(lambda: H.SegConfusion(3).update(_OnDevice(), classes)) == HOT % "SegConfusion target"
    assert _message(lambda: H.label_components(u8)) == MAPS % "label_components map"
    assert _message(lambda: H.label_components(u8.float(), 0.5)) == HOT % "label_components prediction"
    assert _message(lambda: H.clean_mask(u8, None)) == MAPS % "clean_mask map"
    assert _message(lambda: H.component_table(u8.int(), torch.zeros(2, dtype=torch.int32))) == MAPS % "label map"
    assert _message(lambda: H.distance_transform(u8)) == MAPS % "distance_transform map"
    assert _message(lambda: H.skeleton_links(u8)) == MAPS % "skeleton_links map"
    assert _message(lambda: D.select_hist([(u8.int(), u8)])) == MAPS % "value map"
    assert _message(lambda: H.object_metrics(split, 0.5)) == HOT % "prediction to measure"
    assert _message(lambda: H.color_segmaps(logits, x, m, 0.5)) == HOT % "segmentation-map image"
    assert _message(lambda: E._require_device(classes, "evaluation mask")) == EVAL % "evaluation mask"


def test_step_rows_grow_by_doubling_and_keep_order_and_weights():
    from hyperpri_amd.metrics import _StepRows
    for as_float, kind in ((False, int), (True, float)):
        rows = _StepRows(3, "cpu", capacity=2, as_float=as_float)
        for i in range(5):                                  # capacity 2 -> 4 -> 8: the growth rule is crossed twice
            rows.add(10 + i, lambda row, i=i: row.fill_(7 * i + 1))
        assert rows.n == 5 and rows.buf.shape == (8, 3) and int(rows.buf[5:].abs().sum()) == 0
        got, weights = rows.rows()
        assert got == [[7 * i + 1] * 3 for i in range(5)] and weights == [10, 11, 12, 13, 14]
        assert all(type(v) is kind for r in got for v in r)
        weights.append(0)                                   # (a copy: the caller may keep it)
        assert rows.rows()[1] == [10, 11, 12, 13, 14]
        with pytest.raises(ZeroDivisionError):              # a row whose fill raises does not count
            rows.add(99, lambda row: 1 // 0)
        assert rows.n == 5 and len(rows.weights) == 5
        rows.reset()
        assert rows.rows() == ([], []) and rows.n == 0 and int(rows.buf.abs().sum()) == 0


def test_the_step_buffers_of_the_model_are_that_buffer():
    from hyperpri_amd.metrics import _StepConfusion, _StepCounts, _StepRows
    c, k = _StepCounts(0.25, "cpu"), _StepConfusion(3, 255, "cpu")
    assert isinstance(c, _StepRows) and c.threshold == 0.25 and c.buf.shape == (256, 4) and c.as_float
    assert isinstance(k, _StepRows) and (k.K, k.ignore_index) == (3, 255) and k.buf.shape == (256, 10) and not k.as_float
    assert _message(lambda: c.update(torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, 4, 4))) == HOT % "prediction"
    assert _message(lambda: k.update(torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4))) == HOT % "prediction"
    with pytest.raises(ValueError, match=r"^SegmentationModel: built for 3 classes, got logits \(1, 4, 4, 4\)$"):
        k.update(_OnDevice(K=4), torch.zeros(1, 4, 4))
    assert c.n == 0 and k.n == 0


def test_as_f32_returns_fp32_input_itself():
    from hyperpri_amd._args import _as_f32, _grad_f32
    x = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    assert _as_f32(x) is x and _as_f32(x.t()).data_ptr() == x.data_ptr()       # no copy, not even for a strided view
    for other in (x.to(torch.float64), x.to(torch.int64), x.to(torch.uint8), x.to(torch.bfloat16), x > 2):
        y = _as_f32(other)
        assert y.dtype == torch.float32 and y.shape == other.shape and torch.equal(y, other.to(torch.float64).float())
    g = _grad_f32(x.t().to(torch.float64))
    assert g.dtype == torch.float32 and g.is_contiguous() and torch.equal(g, x.t())
    assert _grad_f32(x) is x                                # a contiguous fp32 gradient is passed on as it is
