"""Host-side checks of the evaluation module (hyperpri_amd/evaluate.py) and of its kernel's launcher (csrc/segmap.hip): argument
errors come back as error codes before any launch, CPU tensors are refused loudly, and the reference's last-point patch of the
precision-recall curve (PLTrainer.py:598-600) is applied exactly when its condition holds.  No GPU needed."""
import ctypes

import pytest
import torch

from hyperpri_amd import evaluate as E

PAL = [v for colour in E.PALETTE for v in colour]


def _overlay(lib, image=1, pred=1, mask=1, rgb=1, strides=(48, 16, 4, 1), C=3, bands=(0, 1, 2), N=1, h=4, w=4, gamma=2.2,
             inv_gamma=1 / 2.2, alpha=0.6, pal=PAL):
    """hpri_segmap_overlay with one argument made bad; the good pointers are a live host buffer, which a launcher that validates
    first never passes on."""
    buf = (ctypes.c_float * 64)()
    ptr = lambda ok: ctypes.c_void_p(ctypes.addressof(buf) if ok else 0)      # noqa: E731
    return lib.hpri_segmap_overlay(ptr(image), *strides, C, *bands, ptr(pred), ptr(mask), N, h, w, 0.5, 1, gamma, inv_gamma, alpha,
                                   *pal, ptr(rgb), ctypes.c_void_p(0), ctypes.c_void_p(0))


def test_segmap_overlay_rejects_bad_arguments_without_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    for which in ("image", "pred", "mask", "rgb"):
        assert _overlay(lib, **{which: 0}) == -1, which
        assert b"null" in lib.hpri_last_error()
    for bands in ((3, 1, 2), (0, 3, 2), (0, 1, 3), (-1, 1, 2), (0, 1, 238)):
        assert _overlay(lib, bands=bands) == -1, bands
        assert b"band" in lib.hpri_last_error()
    assert _overlay(lib, C=238, strides=(238 * 16, 16, 4, 1), bands=(125, 49, 238)) == -1
    for gamma in (0.0, -2.2, float("nan")):
        assert _overlay(lib, gamma=gamma) == -1, gamma
        assert b"gamma" in lib.hpri_last_error()
    for alpha in (-0.01, 1.01, float("nan")):
        assert _overlay(lib, alpha=alpha) == -1, alpha
        assert b"alpha" in lib.hpri_last_error()
    for size in ({"N": 0}, {"h": 0}, {"w": -4}, {"C": 0}):
        assert _overlay(lib, **size) == -1, size
        assert b"size" in lib.hpri_last_error()
    assert _overlay(lib, strides=(48, 16, -4, 1)) == -1
    assert _overlay(lib, pal=[1.5] + PAL[1:]) == -1
    with pytest.raises(RuntimeError, match="hpri_segmap_overlay failed"):
        _lib.call("hpri_segmap_overlay", None, 48, 16, 4, 1, 3, 0, 1, 2, None, None, 1, 4, 4, 0.5, 1, 2.2, 1 / 2.2, 0.6, *PAL, None, None,
                  None)


def test_predict_split_and_color_segmaps_refuse_cpu_tensors():
    import hyperpri_amd as H
    net = torch.nn.Conv2d(3, 1, 1)
    batch = {"image": torch.zeros(1, 3, 4, 4), "mask": torch.zeros(1, 1, 4, 4), "index": ["a"]}
    net.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.predict_split(net, [batch])
    assert net.training                                            # the mode comes back when the pass raises, too
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.color_segmaps(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), 0.5)
    with pytest.raises(ValueError, match="no batches"):
        H.predict_split(net, [])


def test_last_point_patch_applies_only_under_its_condition():
    prec = torch.tensor([0.1, 0.4, 0.7, 0.8, 0.0, 1.0])
    got = E.patch_last_point(prec)
    assert torch.equal(got, torch.tensor([0.1, 0.4, 0.7, 0.8, (1 + torch.tensor(0.8)) / 2, 1.0]))
    assert prec[-2] == 0.0                                        # a copy: the caller's curve is left alone
    fine = torch.tensor([0.1, 0.4, 0.7, 0.8, 0.95, 1.0])
    assert torch.equal(E.patch_last_point(fine), fine)
    edge = torch.tensor([0.1, 0.4, 0.7, 0.8, 1e-5, 1.0])          # small, but not below 1e-6
    assert torch.equal(E.patch_last_point(edge), edge)


def test_public_names_and_defaults():
    import hyperpri_amd as H
    for name in ("predict_split", "validate_net", "test_net", "color_segmaps", "write_segmaps", "SplitPrediction"):
        assert getattr(H, name) is getattr(E, name)
    assert E.PALETTE == ((202 / 255, 0.0, 32 / 255), (5 / 255, 133 / 255, 176 / 255), (155 / 255, 191 / 255, 133 / 255))
    assert (E.ALPHA, E.HSI_BANDS, E.HSI_GAMMA, E.RGB_BANDS, E.RGB_GAMMA) == (0.6, (125, 49, 0), 2.2, (0, 1, 2), 1.0)
