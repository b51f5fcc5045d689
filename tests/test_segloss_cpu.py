"""Host-side checks of the imbalance-aware binary losses (csrc/segloss.hip, hyperpri_amd/trainer.py): the C ABI declares and exports
the entry points, the launchers refuse every bad argument before any launch, the constructors map the conventional signatures onto
the family's parameters, and only a default-configured BCEWithLogitsLoss is offered to the head's fused loss.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hpri_seg_loss_workspace_doubles", "hpri_seg_loss_state_doubles", "hpri_seg_loss_fwd", "hpri_seg_loss_bwd")


def test_header_declares_and_both_libraries_export_the_entry_points():
    from hyperpri_amd import _lib
    decls = _lib.parse_header()
    names = set(re.findall(r"\b(hpri_\w+)\s*\(", open(os.path.join(ROOT, "include", "hyperpri_hip.h")).read()))
    assert names == set(decls.keys())                                  # header == what the binding parses
    for lib in (_lib.load(), _lib.load_f16()):
        for name in names:
            assert hasattr(lib, name), name                            # header == exports, still
    for name in ENTRY_POINTS:
        assert name in decls, name
    assert decls["hpri_seg_loss_workspace_doubles"][0] is ctypes.c_size_t and decls["hpri_seg_loss_state_doubles"][0] is ctypes.c_size_t
    assert decls["hpri_seg_loss_fwd"][1].count(ctypes.c_float) == 9 and decls["hpri_seg_loss_bwd"][1].count(ctypes.c_float) == 5


def test_workspace_and_state_helpers_are_pure_host_functions():
    from hyperpri_amd import _lib
    ws, st = _lib.load().hpri_seg_loss_workspace_doubles, _lib.load().hpri_seg_loss_state_doubles
    # four fp64 partial sums per workgroup; a workgroup per 1024 elements of one image, at most 1024 workgroups in all
    assert ws(1, 1) == 4 and ws(1, 1024) == 4 and ws(1, 1025) == 8 and ws(3, 1961) == 4 * 3 * 2
    assert ws(2, 608 * 968) == 4 * 2 * 512 and ws(2, 1 << 40) == 4 * 1024 and ws(3, 1 << 40) == 4 * 3 * 341
    assert ws(1024, 10 ** 6) == 4 * 1024 and ws(5000, 10 ** 6) == 4 * 5000          # beyond 1024 images: one slice each
    assert ws(0, 16) == 0 and ws(2, 0) == 0
    assert st(4, 0) == 3 and st(4, 1) == 9 and st(0, 1) == 0


class _Host:
    """Live host memory for the pointer arguments: a launcher that validates first never passes it on."""

    def __init__(self):
        self.buf = (ctypes.c_double * 64)()

    def p(self, ok=1):
        return ctypes.c_void_p(ctypes.addressof(self.buf) if ok else 0)


GOOD = dict(n_img=2, hw=16, w_point=1.0, pos_weight=1.0, focal_gamma=0.0, focal_alpha=-1.0, mean=1, w_overlap=1.0, alpha=0.5, beta=0.5,
            smooth=1.0, tversky_gamma=1.0, per_image=0, ws=8, st=5)


def _fwd(lib, h, null=(), **kw):
    a = dict(GOOD, **kw)
    p = lambda name: h.p(name not in null)      # noqa: E731
    return lib.hpri_seg_loss_fwd(p("logits"), p("target"), a["n_img"], a["hw"], a["w_point"], a["pos_weight"], a["focal_gamma"],
                                 a["focal_alpha"], a["mean"], a["w_overlap"], a["alpha"], a["beta"], a["smooth"], a["tversky_gamma"],
                                 a["per_image"], p("loss"), p("state"), a["st"], p("terms"), p("workspace"), a["ws"], ctypes.c_void_p(0))


def _bwd(lib, h, null=(), **kw):
    a = dict(GOOD, **kw)
    p = lambda name: h.p(name not in null)      # noqa: E731
    return lib.hpri_seg_loss_bwd(p("logits"), p("target"), a["n_img"], a["hw"], a["w_point"], a["pos_weight"], a["focal_gamma"],
                                 a["focal_alpha"], a["w_overlap"], a["per_image"], p("state"), a["st"], h.p(0), p("dlogits"), ctypes.c_void_p(0))


def test_launchers_reject_bad_arguments_without_launch():
    from hyperpri_amd import _lib
    lib, h = _lib.load(), _Host()
    nan = float("nan")
    for name in ("logits", "target", "loss", "state", "terms", "workspace"):
        assert _fwd(lib, h, null=(name,)) == -1, name
        assert b"null" in lib.hpri_last_error()
    for name in ("logits", "target", "state", "dlogits"):
        assert _bwd(lib, h, null=(name,)) == -1, name
        assert b"null" in lib.hpri_last_error()
    shared = [(dict(n_img=0), b"size"), (dict(n_img=-2), b"size"), (dict(hw=0), b"size"), (dict(hw=-5), b"size"),
              (dict(pos_weight=0.0), b"pos_weight"), (dict(pos_weight=-1.0), b"pos_weight"), (dict(pos_weight=nan), b"pos_weight"),
              (dict(focal_gamma=-0.5), b"focal gamma"), (dict(focal_gamma=nan), b"focal gamma"),
              (dict(focal_alpha=1.25), b"focal alpha"), (dict(focal_alpha=nan), b"focal alpha"),
              (dict(w_point=0.0, w_overlap=0.0), b"both weights"), (dict(w_point=nan), b"both weights")]
    for call in (_fwd, _bwd):
        for kw, msg in shared:
            assert call(lib, h, **kw) == -1, (call.__name__, kw)
            assert msg in lib.hpri_last_error(), (call.__name__, kw, lib.hpri_last_error())
    for kw, msg in [(dict(alpha=-0.1), b"alpha and beta"), (dict(beta=-0.1), b"alpha and beta"), (dict(alpha=0.0, beta=0.0), b"alpha + beta"),
                    (dict(alpha=nan), b"alpha"), (dict(smooth=-1e-3), b"smooth"), (dict(tversky_gamma=0.0), b"tversky gamma"),
                    (dict(tversky_gamma=-1.0), b"tversky gamma"), (dict(tversky_gamma=nan), b"tversky gamma")]:
        assert _fwd(lib, h, **kw) == -1, kw
        assert msg in lib.hpri_last_error(), (kw, lib.hpri_last_error())
    assert _fwd(lib, h, ws=7) == -3 and b"workspace" in lib.hpri_last_error()
    assert _fwd(lib, h, n_img=2, hw=3000, ws=4 * 2 * 3 - 1) == -3
    # a state buffer sized for another per_image / n_img than the call's (st = 5 holds two groups)
    for call in (_fwd, _bwd):
        assert call(lib, h, st=2) == -3 and b"state" in lib.hpri_last_error()
        assert call(lib, h, per_image=1, st=4) == -3 and b"state" in lib.hpri_last_error()
        assert call(lib, h, n_img=3, per_image=1, ws=12) == -3 and b"state" in lib.hpri_last_error()
    with pytest.raises(RuntimeError, match="hpri_seg_loss_bwd failed"):
        _lib.call("hpri_seg_loss_bwd", None, None, 1, 16, 1.0, 1.0, 0.0, -1.0, 0.0, 0, None, 3, None, None, None)


def test_constructors_map_the_conventional_signatures():
    import hyperpri_amd as H
    # config(): (w_point, pos_weight, focal_gamma, focal_alpha, mean, w_overlap, alpha, beta, s, tversky_gamma, per_image)
    assert H.DiceLoss().config() == (0.0, 1.0, 0.0, -1.0, True, 1.0, 0.5, 0.5, 0.5, 1.0, False)
    assert H.DiceLoss(smooth=3.0, per_image=True).config() == (0.0, 1.0, 0.0, -1.0, True, 1.0, 0.5, 0.5, 1.5, 1.0, True)
    assert H.TverskyLoss(0.3, 0.7, 2.0, gamma=0.75, per_image=True).config() == (0.0, 1.0, 0.0, -1.0, True, 1.0, 0.3, 0.7, 2.0, 0.75, True)
    assert H.FocalLoss().config() == (1.0, 1.0, 2.0, 0.25, True, 0.0, 0.5, 0.5, 1.0, 1.0, False)
    assert H.FocalLoss(gamma=1.5, alpha=-1, reduction="sum").config()[:5] == (1.0, 1.0, 1.5, -1.0, False)
    assert H.DiceBCELoss(0.7, 0.3, pos_weight=torch.tensor([4.0]), smooth=2.0).config() == (0.7, 4.0, 0.0, -1.0, True, 0.3, 0.5, 0.5, 1.0, 1.0, False)
    assert H.SegLoss().config() == (1.0, 1.0, 0.0, -1.0, True, 0.0, 0.5, 0.5, 1.0, 1.0, False)
    for cls in (H.DiceLoss, H.TverskyLoss, H.FocalLoss, H.DiceBCELoss):
        assert issubclass(cls, H.SegLoss)
    for bad in (dict(pos_weight=0.0), dict(focal_gamma=-1.0), dict(focal_alpha=1.5), dict(tversky_alpha=-0.1), dict(tversky_alpha=0.0, tversky_beta=0.0),
                dict(smooth=-1.0), dict(tversky_gamma=0.0), dict(bce_weight=0.0), dict(reduction="none"), dict(pos_weight=torch.ones(2))):
        with pytest.raises(ValueError):
            H.SegLoss(**bad)
    with pytest.raises(ValueError, match="reduction"):
        H.BCEWithLogitsLoss(reduction="none")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.DiceLoss()(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.BCEWithLogitsLoss(pos_weight=2.0)(torch.zeros(4), torch.zeros(4))
    assert H.SegLoss().last_terms is None


def test_only_a_default_bce_is_offered_to_the_fused_head():
    import hyperpri_amd as H
    from hyperpri_amd.trainer import _takes_fused_head
    assert H.BCEWithLogitsLoss().fusable and _takes_fused_head(H.BCEWithLogitsLoss())
    assert _takes_fused_head(H.BCEWithLogitsLoss(pos_weight=None, reduction="mean"))
    for crit in (H.BCEWithLogitsLoss(pos_weight=3.0), H.BCEWithLogitsLoss(pos_weight=torch.tensor(1.0)), H.BCEWithLogitsLoss(reduction="sum"),
                 H.SegLoss(), H.DiceBCELoss(), H.DiceLoss(), torch.nn.BCEWithLogitsLoss()):
        assert not _takes_fused_head(crit), crit

    class Mine(H.BCEWithLogitsLoss):
        pass
    assert not _takes_fused_head(Mine())                              # a subclass may compute anything
    weighted = H.BCEWithLogitsLoss(pos_weight=3.0, reduction="sum")
    assert (weighted.pos_weight, weighted.reduction) == (3.0, "sum") and weighted._seg.config()[:5] == (1.0, 3.0, 0.0, -1.0, False)
    model = H.SegmentationModel(torch.nn.Conv2d(3, 1, 1), weighted)
    assert model.f_criterion is weighted


# ---------------------------------------------------------------------------------------------------
# the numbers behind the GPU tests' gradient gates: the closed form in fp32 torch on the CPU against the fp64 reference
# (both from tests/test_gpu_segloss.py; nothing here runs the HIP kernels)
# ---------------------------------------------------------------------------------------------------
def test_closed_form_in_fp32_on_the_cpu_stays_inside_the_gate():
    """The number behind the focal cases' rtol (docstring of tests/test_gpu_segloss.py): the closed form in fp32 torch against fp64, worst element."""
    import test_gpu_segloss as G
    for config in ("focal", "focal15_pw"):
        for name in G.SHAPES:
            _, p, g = G.CONFIGS[config]
            _, _, _, _, a, b = G._reference(name, config)
            x, y = G._inputs(name)
            err = (G._closed_form32(x, y, p, g).double() - (a + b)).abs()
            worst = float((err / (G.RTOL * (a.abs() + b.abs()) + 1e-30)).max())
            print(f"closed form fp32 (CPU) {name} {config}: gradient error / allowance {worst:.3f}")
            assert worst <= 0.5


def test_closed_form_in_fp32_on_the_cpu_pins_the_soft_label_bound():
    """The numbers behind the soft-label bound (docstring of tests/test_gpu_segloss.py), on uniform soft labels at (3, 1, 37, 53): the closed form in fp32
    torch on the CPU stays within 0.05 to 0.12 of rtol times the sum of the magnitudes (asserted: at most half of it, so that twice
    its error fits), while under the pointwise terms it misses the gate relative to |a_i| + |b_i| by factors of 2.6 (weighted BCE),
    4.9 (gamma 1.5) and 12 (focal): no fp32 evaluation can meet that gate where the gradient crosses zero."""
    import test_gpu_segloss as G
    name = "3x1x37x53"
    for config in ("wbce", "focal", "focal15_pw", "dice_batch", "focal_tversky_img", "dicebce"):
        _, p, g = G.CONFIGS[config]
        _, _, _, _, a, b = G._reference(name, config, "uniform")
        x, y = G._inputs(name, "uniform")
        err = (G._closed_form32(x, y, p, g).double() - (a + b)).abs()
        wide = float((err / (G.RTOL * G._magnitudes(x.double(), y.double(), p, g) + 1e-30)).max())
        strict = float((err / (G.RTOL * (a.abs() + b.abs()) + 1e-30)).max())
        print(f"closed form fp32 (CPU) uniform soft labels {config}: error / (rtol * magnitudes) {wide:.3f}, error / strict allowance {strict:.2f}")
        assert wide <= 0.5
        if p["wo"] == 0:
            assert strict > 2.0
