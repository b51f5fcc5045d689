"""Host-side checks of the multi-class tail (csrc/multiclass.hip, hpri_segmap_classes, hyperpri_amd/trainer.py, evaluate.py): the
C ABI declares and exports the entry points, their launchers refuse bad arguments before any launch, the metrics of a confusion
matrix match a numpy restatement, CPU tensors are refused loudly and the binary defaults are where they were.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

ENTRY_POINTS = ("hpri_softmax_ce_workspace_doubles", "hpri_softmax_ce_fwd", "hpri_softmax_ce_bwd", "hpri_seg_confusion",
                "hpri_segmap_classes")


def test_header_declares_and_both_libraries_export_the_entry_points():
    from hyperpri_amd import _lib
    decls = _lib.parse_header()
    for lib in (_lib.load(), _lib.load_f16()):
        for name in ENTRY_POINTS:
            assert name in decls, name
            assert hasattr(lib, name), name
    assert decls["hpri_softmax_ce_workspace_doubles"][0] is ctypes.c_size_t


def test_workspace_helper_is_a_pure_host_function():
    from hyperpri_amd import _lib
    ws = _lib.load().hpri_softmax_ce_workspace_doubles
    # three fp64 partial sums (loss, weight, invalid count) per block of 256 lanes, at most 1024 blocks
    assert ws(1) == 3 and ws(256) == 3 and ws(257) == 6
    assert ws(2 * 608 * 968) == 3 * 1024 and ws(1 << 40) == 3 * 1024
    assert [ws(n) for n in (15, 3600, 10 ** 6)] == [ws(n) for n in (15, 3600, 10 ** 6)]


class _Host:
    """Live host memory for the pointer arguments: a launcher that validates first never passes it on."""

    def __init__(self):
        self.buf = (ctypes.c_double * 64)()

    def p(self, ok=1):
        return ctypes.c_void_p(ctypes.addressof(self.buf) if ok else 0)


def _fwd(lib, h, K=3, N=1, HW=16, kind=0, ws=3, **null):
    p = lambda name: h.p(name not in null)      # noqa: E731
    return lib.hpri_softmax_ce_fwd(p("logits"), p("target"), kind, h.p(0), N, K, HW, 0, 0, 1, p("loss"), p("lse"), p("denom"), h.p(0),
                                   p("workspace"), ws, ctypes.c_void_p(0))


def _bwd(lib, h, K=3, N=1, HW=16, kind=0, **null):
    p = lambda name: h.p(name not in null)      # noqa: E731
    return lib.hpri_softmax_ce_bwd(p("logits"), p("lse"), p("target"), kind, h.p(0), N, K, HW, 0, 0, p("denom"), h.p(0), p("dlogits"),
                                   ctypes.c_void_p(0))


def _conf(lib, h, K=3, N=1, HW=16, kind=0, **null):
    p = lambda name: h.p(name not in null)      # noqa: E731
    return lib.hpri_seg_confusion(p("logits"), p("target"), kind, N, K, HW, 0, 0, p("counts"), p("classes"), ctypes.c_void_p(0))


def test_cross_entropy_and_confusion_reject_bad_arguments_without_launch():
    from hyperpri_amd import _lib
    lib, h = _lib.load(), _Host()
    for name in ("logits", "target", "loss", "lse", "denom", "workspace"):
        assert _fwd(lib, h, **{name: 0}) == -1, name
        assert b"null" in lib.hpri_last_error()
    for name in ("logits", "lse", "target", "denom", "dlogits"):
        assert _bwd(lib, h, **{name: 0}) == -1, name
        assert b"null" in lib.hpri_last_error()
    assert _conf(lib, h, logits=0) == -1 and b"null" in lib.hpri_last_error()
    assert _conf(lib, h, target=0) == -1 and b"together" in lib.hpri_last_error()      # counts without a target
    assert _conf(lib, h, counts=0) == -1 and b"together" in lib.hpri_last_error()
    assert _conf(lib, h, target=0, counts=0, classes=0) == -1                             # nothing asked for
    for call in (_fwd, _bwd, _conf):
        for K in (1, 65, 0, -3):
            assert call(lib, h, K=K) != 0, (call.__name__, K)
            assert b"classes must lie in [2, 64]" in lib.hpri_last_error()
        assert call(lib, h, N=0) == -1 and b"size" in lib.hpri_last_error()
        assert call(lib, h, HW=0) == -1 and b"size" in lib.hpri_last_error()
        assert call(lib, h, kind=3) == -1 and b"target kind" in lib.hpri_last_error()
    assert _fwd(lib, h, ws=2) == -3 and b"workspace" in lib.hpri_last_error()
    with pytest.raises(RuntimeError, match="hpri_seg_confusion failed"):
        _lib.call("hpri_seg_confusion", None, None, 0, 1, 3, 16, 0, 0, None, None, None)


def _classes(lib, h, K=4, pal=None, strides=(48, 16, 4, 1), C=3, bands=(0, 1, 2), N=1, h_=4, w=4, gamma=2.2, alpha=0.6, **null):
    p = lambda name: h.p(name not in null)      # noqa: E731
    table = (ctypes.c_float * (3 * 64))(*(pal if pal is not None else [0.5] * (3 * 64)))
    palette = ctypes.cast(table, ctypes.c_void_p) if "palette" not in null else ctypes.c_void_p(0)
    return lib.hpri_segmap_classes(p("image"), *strides, C, *bands, p("classes"), N, h_, w, gamma, 1 / gamma if gamma else 0.0, alpha,
                                   palette, K, p("rgb"), ctypes.c_void_p(0))


def test_segmap_classes_rejects_bad_arguments_without_launch():
    from hyperpri_amd import _lib
    lib, h = _lib.load(), _Host()
    for name in ("image", "classes", "palette", "rgb"):
        assert _classes(lib, h, **{name: 0}) == -1, name
        assert b"null" in lib.hpri_last_error()
    for K in (1, 65):
        assert _classes(lib, h, K=K) == -1 and b"classes must lie in [2, 64]" in lib.hpri_last_error()
    assert _classes(lib, h, bands=(0, 3, 2)) == -1 and b"band" in lib.hpri_last_error()
    assert _classes(lib, h, gamma=0.0) == -1 and b"gamma" in lib.hpri_last_error()
    assert _classes(lib, h, alpha=1.5) == -1 and b"alpha" in lib.hpri_last_error()
    assert _classes(lib, h, w=0) == -1 and b"size" in lib.hpri_last_error()
    assert _classes(lib, h, strides=(48, 16, -4, 1)) == -1
    bad = [0.5] * (3 * 64)
    bad[3 * 3 + 1] = 1.25                                     # inside the K = 4 rows that count
    assert _classes(lib, h, pal=bad) == -1 and b"palette" in lib.hpri_last_error()
    bad = [0.5] * (3 * 64)
    bad[3 * 4] = float("nan")                                 # the first entry of the K = 5 rows' last one
    assert _classes(lib, h, K=5, pal=bad) == -1 and b"palette" in lib.hpri_last_error()


def _restate(c):
    """The documented definitions over C[t][p], in numpy."""
    c = np.asarray(c, dtype=np.float64)
    row, col, diag = c.sum(1), c.sum(0), np.diag(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = diag / (row + col - diag)
        dice = 2 * diag / (row + col)
    return diag.sum() / c.sum(), iou, dice, np.nanmean(iou), np.nanmean(dice)


def test_metrics_from_confusion_match_a_numpy_restatement():
    import hyperpri_amd as H
    # class 2 is absent from the truth (row) and from the prediction (column): nan, and left out of the means
    c = [[50, 3, 0, 2], [4, 20, 0, 6], [0, 0, 0, 0], [1, 5, 0, 9]]
    m = H.multiclass_metrics_from_confusion(c)
    acc, iou, dice, miou, mdice = _restate(c)
    assert m["acc"] == pytest.approx(acc, rel=1e-12) and acc == 79 / 100
    assert np.isnan(m["iou_per_class"][2]) and np.isnan(m["dice_per_class"][2])
    np.testing.assert_allclose(m["iou_per_class"], iou, rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(m["dice_per_class"], dice, rtol=1e-12, equal_nan=True)
    assert m["mean_iou"] == pytest.approx(miou, rel=1e-12) and m["mean_dice"] == pytest.approx(mdice, rel=1e-12)
    assert m["mean_iou"] == pytest.approx((50 / 60 + 20 / 38 + 9 / 23) / 3, rel=1e-12)
    assert np.array_equal(m["confusion"], np.asarray(c)) and m["confusion"].dtype == np.int64
    # tensors are taken as they are; an empty matrix has no defined value anywhere
    assert H.multiclass_metrics_from_confusion(torch.tensor(c))["mean_dice"] == m["mean_dice"]
    empty = H.multiclass_metrics_from_confusion(np.zeros((3, 3), dtype=np.int64))
    assert all(np.isnan(empty[k]) for k in ("acc", "mean_iou", "mean_dice"))
    with pytest.raises(ValueError, match="square"):
        H.multiclass_metrics_from_confusion([[1, 2, 3], [4, 5, 6]])


def test_cpu_tensors_and_bad_options_fail_loudly():
    import hyperpri_amd as H
    logits, target = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.CrossEntropyLoss()(logits, target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.SegConfusion(3).update(logits, target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.argmax_classes(logits)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.color_classmaps(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))
    net = torch.nn.Conv2d(3, 3, 1).train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.evaluate_multiclass(net, [{"image": logits, "mask": target, "index": ["a"]}], 3)
    assert net.training                                            # the mode comes back when the pass raises
    with pytest.raises(ValueError, match="no batches"):
        H.evaluate_multiclass(net, [], 3)
    with pytest.raises(ValueError, match="reduction"):
        H.CrossEntropyLoss(reduction="none")
    for K in (1, 65):
        with pytest.raises(ValueError, match="classes"):
            H.SegConfusion(K)
        with pytest.raises(ValueError, match="classes"):
            H.evaluate_multiclass(net, [], K)
    crit = H.CrossEntropyLoss(weight=torch.tensor([1.0, 2.0, 0.5]), ignore_index=255, reduction="sum")
    assert "weight" in dict(crit.named_buffers()) and (crit.ignore_index, crit.reduction) == (255, "sum")
    assert (H.CrossEntropyLoss().weight, H.CrossEntropyLoss().ignore_index, H.CrossEntropyLoss().reduction) == (None, -100, "mean")


def test_segmentation_model_defaults_stay_binary():
    import hyperpri_amd as H
    net = torch.nn.Conv2d(3, 1, 1)
    model = H.SegmentationModel(net)
    assert model.task == "binary" and model.num_classes == 1 and type(model.f_criterion) is H.BCEWithLogitsLoss
    assert H.SegmentationModel(net, None, "SGD", 1e-2, 0.0, 0.9, 0.4).threshold == 0.4          # the positional arguments of before
    multi = H.SegmentationModel(torch.nn.Conv2d(3, 4, 1), task="multiclass", num_classes=4)
    assert multi.task == "multiclass" and type(multi.f_criterion) is H.CrossEntropyLoss and multi.num_classes == 4
    with pytest.raises(ValueError, match="task"):
        H.SegmentationModel(net, task="multilabel")
    with pytest.raises(ValueError, match="num_classes"):
        H.SegmentationModel(net, task="multiclass")
    assert multi.epoch_metrics("val") == {}


def test_default_class_palette_is_distinct_and_in_range():
    import hyperpri_amd as H
    from hyperpri_amd import evaluate as E
    for K in (2, 4, 11, 64):
        pal = H.default_class_palette(K)
        assert len(pal) == K and len(set(pal[1:])) == K - 1
        assert all(len(row) == 3 and all(0.0 <= v <= 1.0 for v in row) for row in pal)
    assert H.default_class_palette(4)[1:] == E.PALETTE
    for name in ("CrossEntropyLoss", "SegConfusion", "multiclass_metrics_from_confusion", "argmax_classes", "evaluate_multiclass",
                 "color_classmaps"):
        assert hasattr(H, name), name
