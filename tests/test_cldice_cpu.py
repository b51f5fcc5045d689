"""The centerline loss without a GPU: ``soft_skeleton_reference`` (the numpy restatement of the contract of csrc/skeleton.hip, tie rules
included) against torch autograd of the PUBLISHED formulation of clDice (Shit et al., CVPR 2021), written out below with max_pool2d;
the launchers' argument checks through the C ABI; the constructor of ``clDiceLoss``; the compiler's report for the new kernels.

Tie-free inputs: a permutation of k / (n + 1), k = 1 .. n, mapped into [0.02, 0.98].  On such inputs every subgradient choice of a
min or a max leads back to the same input pixel (the eroded planes hold COPIES of input values, and all copies of a value route to
its one source), so the first-optimum rule of the contract and torch's own choices agree up to summation order: values must be equal
in fp64, gradients agree to 1e-12."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the published code (cldice_loss/pytorch/soft_skeleton.py of the paper's repository), 2-D branch ---------------------------------
def soft_erode(img):
    p1 = -F.max_pool2d(-img, (3, 1), (1, 1), (1, 0))
    p2 = -F.max_pool2d(-img, (1, 3), (1, 1), (0, 1))
    return torch.min(p1, p2)


def soft_dilate(img):
    return F.max_pool2d(img, (3, 3), (1, 1), (1, 1))


def soft_open(img):
    return soft_dilate(soft_erode(img))


def soft_skel(img, iter_):
    img1 = soft_open(img)
    skel = F.relu(img - img1)
    for _ in range(iter_):
        img = soft_erode(img)
        img1 = soft_open(img)
        delta = F.relu(img - img1)
        skel = skel + F.relu(delta - skel * delta)
    return skel


def tie_free(shape, seed):
    n = int(np.prod(shape))
    rng = np.random.RandomState(seed)
    return (0.02 + 0.96 * (rng.permutation(n) + 1.0) / (n + 1)).reshape(shape)


@pytest.mark.parametrize("shape,iters", [((37, 53), 5), ((16, 24), 3), ((5, 3), 2), ((70, 131), 10)])
def test_reference_matches_autograd_of_the_published_formulation(shape, iters):
    from hyperpri_amd import soft_skeleton_reference
    p = tie_free((2,) + shape, 11 + iters)
    g = np.random.RandomState(5).uniform(-1, 1, size=p.shape)
    S, gp, A = soft_skeleton_reference(p, iters, grad=g)
    t = torch.from_numpy(p).unsqueeze(1).requires_grad_(True)
    ref = soft_skel(t, iters)
    ref.backward(torch.from_numpy(g).unsqueeze(1))
    assert S.dtype == np.float64 and np.array_equal(S, ref.detach().numpy()[:, 0])
    err = np.abs(gp - t.grad.numpy()[:, 0]).max()
    print(f"{shape}/{iters}: max |gp - autograd| {err:.2e}, max |gp| {np.abs(gp).max():.2e}")
    assert err <= 1e-12
    assert (A >= np.abs(gp) - 1e-15).all()              # the absolute run bounds the signed one
    assert np.array_equal(soft_skeleton_reference(p, iters), S)


def test_reference_forward_on_a_binary_two_bar_mask():
    """Forward values do not depend on ties: a plateau input must give the published values exactly."""
    from hyperpri_amd import soft_skeleton_reference
    m = np.zeros((24, 31))
    m[3:8, 2:29] = 1          # a bar five pixels thick
    m[12:21, 20:23] = 1       # a bar three pixels wide
    for iters in (0, 1, 3, 6):
        S = soft_skeleton_reference(m, iters)
        ref = soft_skel(torch.from_numpy(m)[None, None], iters)[0, 0].numpy()
        assert np.array_equal(S, ref), iters
        S32 = soft_skeleton_reference(m.astype(np.float32), iters, dtype=np.float32)
        assert S32.dtype == np.float32 and np.array_equal(S32.astype(np.float64), ref), iters
    assert soft_skeleton_reference(m, 6).sum() > 0


def test_reference_tie_rule_first_optimum_in_scan_order():
    """A constant plane: every min and max ties.  d_0 = 0 everywhere, so no gradient passes (relu'(0) = 0); with one raised pixel
    the erosion's gradient of the FIRST minimum (N before W before C) is what arrives."""
    from hyperpri_amd import soft_skeleton_reference
    p = np.full((5, 5), 0.5)
    _, gp, A = soft_skeleton_reference(p, 2, grad=np.ones_like(p))
    assert not gp.any() and not A.any()
    p[2, 2] = 1.0                                          # S_0 = relu(I_0 - D(E(I_0))): only the peak stands out, by 0.5
    S, gp, _ = soft_skeleton_reference(p, 0, grad=np.ones_like(p))
    assert S[2, 2] == 0.5 and S.sum() == 0.5
    # d_0[2,2] = p[2,2] - I_1[argmax of the window of (2,2)]; I_1 is 0.5 everywhere, its first maximum in the window is (1,1), whose
    # erosion takes its first minimum: its N neighbour (0,1)
    want = np.zeros_like(p)
    want[2, 2], want[0, 1] = 1.0, -1.0
    assert np.array_equal(gp, want)


# -- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_launchers_reject_bad_arguments_before_any_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null, ptr = ctypes.c_void_p(0), ctypes.c_void_p(256)           # (never dereferenced: every call below is refused)
    T = lib.hpri_soft_skeleton_tile()
    assert T == 64 and lib.hpri_soft_skeleton_max_iters() == 32
    assert lib.hpri_soft_skeleton_saved_floats(2, 5, 7, 3) == 7 * 2 * 5 * 7
    assert lib.hpri_soft_skeleton_saved_floats(2, 5, 7, 33) == 0 and lib.hpri_soft_skeleton_saved_floats(0, 5, 7, 3) == 0
    assert lib.hpri_soft_skeleton_workspace_floats(2, 5, 7) == 4 * 2 * 5 * 7
    assert lib.hpri_cldice_workspace_doubles(2, T + 1, 2 * T) == 4 * 2 * 2 * 2
    assert lib.hpri_cldice_state_doubles(3, 1) == 9 and lib.hpri_cldice_state_doubles(3, 0) == 3
    # two planes of (T + 2 (iters + 2))^2 floats fit the 160 KB of a compute unit up to iters = 32
    assert lib.hpri_soft_skeleton_lds_bytes(32) == 2 * 132 * 132 * 4 <= 160 * 1024 and lib.hpri_soft_skeleton_lds_bytes(33) == 0

    def refused(rc, word):
        assert rc == -1, rc
        assert word in lib.hpri_last_error().decode(), lib.hpri_last_error()
    big = 1 << 40
    # soft_skeleton_fwd(p, N, h, w, iters, S, saved, saved_floats, stream)
    refused(lib.hpri_soft_skeleton_fwd(null, 1, 4, 4, 2, ptr, null, 0, null), "null")
    refused(lib.hpri_soft_skeleton_fwd(ptr, 1, 4, 4, 2, null, null, 0, null), "null")
    for N, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        refused(lib.hpri_soft_skeleton_fwd(ptr, N, h, w, 2, ptr, null, 0, null), "sizes")
    refused(lib.hpri_soft_skeleton_fwd(ptr, 40000, 4, 4, 2, ptr, null, 0, null), "beyond")
    refused(lib.hpri_soft_skeleton_fwd(ptr, 1, 50000, 50000, 2, ptr, null, 0, null), "beyond")
    refused(lib.hpri_soft_skeleton_fwd(ptr, 1, (1 << 30) + 1, 1, 2, ptr, null, 0, null), "beyond")
    assert lib.hpri_cldice_workspace_doubles(1, 2 ** 31 - 1, 1) == 4 * 2 ** 25          # (the size functions take any int)
    for iters in (-1, 33):
        refused(lib.hpri_soft_skeleton_fwd(ptr, 1, 4, 4, iters, ptr, null, 0, null), "iters")
    refused(lib.hpri_soft_skeleton_fwd(ptr, 1, 4, 4, 2, ptr, ptr, 5 * 16 - 1, null), "saved")
    # soft_skeleton_bwd(p, saved, saved_floats, grad_S, N, h, w, iters, grad_p, workspace, ws_floats, stream)
    good = [ptr, ptr, big, ptr, 1, 4, 4, 2, ptr, ptr, big, null]
    for i in (0, 1, 3, 8, 9):
        refused(lib.hpri_soft_skeleton_bwd(*[null if k == i else v for k, v in enumerate(good)]), "null")
    for i, v, word in ((4, 0, "sizes"), (5, 0, "sizes"), (6, 0, "sizes"), (7, -1, "iters"), (7, 33, "iters"), (2, 5 * 16 - 1, "saved"),
                       (10, 4 * 16 - 1, "workspace")):
        refused(lib.hpri_soft_skeleton_bwd(*[v if k == i else a for k, a in enumerate(good)]), word)
    # cldice_fwd(logits, target, N, h, w, iters, smooth, per_image, weight, base_loss, base_weight, p, Sp, Sy, saved, saved_floats,
    #            loss, terms, state, state_doubles, workspace, ws_doubles, stream): base_loss and Sp may be null
    good = [ptr, ptr, 2, 4, 4, 2, 1.0, 1, 0.5, null, 0.5, ptr, null, ptr, ptr, big, ptr, ptr, ptr, big, ptr, big, null]
    for i in (0, 1, 11, 13, 14, 16, 17, 18, 20):
        refused(lib.hpri_cldice_fwd(*[null if k == i else v for k, v in enumerate(good)]), "null")
    for i, v, word in ((2, 0, "sizes"), (3, 0, "sizes"), (4, 0, "sizes"), (5, -1, "iters"), (5, 33, "iters"), (6, -0.5, "smooth"),
                       (8, float("nan"), "NaN"), (15, 5 * 32 - 1, "saved"), (19, 5, "state"), (21, 7, "workspace")):
        refused(lib.hpri_cldice_fwd(*[v if k == i else a for k, a in enumerate(good)]), word)
    # cldice_bwd(logits, target, p, Sy, saved, saved_floats, N, h, w, iters, per_image, state, state_doubles, grad_out, base_weight,
    #            grad_base, dlogits, workspace, ws_floats, stream): grad_out and grad_base may be null
    good = [ptr, ptr, ptr, ptr, ptr, big, 2, 4, 4, 2, 1, ptr, big, null, 0.5, null, ptr, ptr, big, null]
    for i in (0, 1, 2, 3, 4, 11, 16, 17):
        refused(lib.hpri_cldice_bwd(*[null if k == i else v for k, v in enumerate(good)]), "null")
    for i, v, word in ((6, 0, "sizes"), (7, 0, "sizes"), (8, 0, "sizes"), (9, -1, "iters"), (9, 33, "iters"), (5, 5 * 32 - 1, "saved"),
                       (12, 5, "state"), (18, 4 * 32 - 1, "workspace")):
        refused(lib.hpri_cldice_bwd(*[v if k == i else a for k, a in enumerate(good)]), word)
    # centerline_counts(skel_pred, skel_truth, pred, truth, N, per_image, counts, stream)
    good = [ptr, ptr, ptr, ptr, 1, 16, ptr, null]
    for i in (0, 1, 2, 3, 6):
        refused(lib.hpri_centerline_counts(*[null if k == i else v for k, v in enumerate(good)]), "null")
    for i, v in ((4, 0), (5, 0), (5, 1 << 31)):
        refused(lib.hpri_centerline_counts(*[v if k == i else a for k, a in enumerate(good)]), "sizes")


# -- the module --------------------------------------------------------------------------------------------------------------------
def test_constructor_mappings_and_checks():
    import hyperpri_amd as H
    from hyperpri_amd import trainer as T
    c = H.clDiceLoss()
    assert (c.iters, c.alpha, c.smooth, c.per_image) == (3, 0.5, 1.0, False)
    assert type(c.base) is H.DiceLoss and c.base.config() == H.DiceLoss(1.0).config()          # (2I + 1) / (P + Y + 1): s = 1/2
    c = H.clDiceLoss(iters=10, alpha=0.3, smooth=0.0, per_image=True)
    assert c.base.config() == H.DiceLoss(0.0, per_image=True).config() and c.base.per_image and c.base.smooth == 0.0
    for base in (H.DiceBCELoss(pos_weight=3.0), H.FocalLoss(), H.TverskyLoss(0.3, 0.7), H.BCEWithLogitsLoss(), H.BCEWithLogitsLoss(pos_weight=2.0)):
        assert H.clDiceLoss(base=base).base is base
    with pytest.raises(TypeError, match="base"):
        H.clDiceLoss(base=torch.nn.BCEWithLogitsLoss())
    for bad in (dict(iters=-1), dict(iters=33), dict(iters=2.5), dict(iters=True), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")),
                dict(smooth=-1.0), dict(smooth=float("nan"))):
        with pytest.raises(ValueError):
            H.clDiceLoss(**bad)
    with pytest.raises(ValueError, match="iters"):
        H.soft_skeleton(torch.zeros(1, 4, 4), 33)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.soft_skeleton(torch.zeros(1, 4, 4), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.clDiceLoss()(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))
    # never the fused head: that path computes the unweighted BCE alone
    for crit in (H.clDiceLoss(), H.clDiceLoss(alpha=0.0, base=H.BCEWithLogitsLoss()), H.clDiceLoss(base=H.BCEWithLogitsLoss())):
        assert not T._takes_fused_head(crit)
    assert "iters=3" in repr(H.clDiceLoss())


def test_alpha_zero_is_the_base_alone_and_launches_no_skeleton_kernel(monkeypatch):
    import hyperpri_amd as H
    from hyperpri_amd import trainer as T
    calls = []
    monkeypatch.setattr(T._lib, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(T._clDiceFn, "apply", lambda *a: pytest.fail("the centerline term was evaluated"))
    sentinel = torch.tensor(0.25)

    class Base(H.SegLoss):
        def forward(self, input, target):       # noqa: A002
            calls.append("base")
            return sentinel
    crit = H.clDiceLoss(alpha=0.0, base=Base())
    assert crit(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)) is sentinel          # the base's own tensor: its bits, its graph
    assert calls == ["base"]


def test_alpha_one_does_not_evaluate_the_base(monkeypatch):
    import hyperpri_amd as H
    from hyperpri_amd import trainer as T
    seen = []

    class Base(H.SegLoss):
        def forward(self, input, target):       # noqa: A002
            pytest.fail("the base was evaluated")
    monkeypatch.setattr(T._clDiceFn, "apply", lambda x, y, base, cfg: (seen.append((base, cfg)), (torch.tensor(1.0), torch.zeros(3)))[1])
    H.clDiceLoss(iters=4, alpha=1.0, smooth=0.5, base=Base(), per_image=True)(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))
    assert seen == [(None, (4, 0.5, True, 1.0, 0.0))]


def test_hard_metric_from_counts():
    from hyperpri_amd.distance import centerline_from_counts
    m = centerline_from_counts([[10, 5, 8, 8], [0, 0, 4, 0], [3, 0, 2, 0]])
    assert m["tprec"][0] == 0.5 and m["tsens"][0] == 1.0 and m["cldice"][0] == pytest.approx(2 * 0.5 / 1.5)
    assert np.isnan(m["tprec"][1]) and m["tsens"][1] == 0.0 and np.isnan(m["cldice"][1])
    assert m["tprec"][2] == 0.0 and np.isnan(m["cldice"][2])                         # tprec + tsens == 0
    assert m["pooled"]["tprec"] == 5 / 13 and m["pooled"]["tsens"] == 8 / 14


# -- the compiler's report ---------------------------------------------------------------------------------------------------------
def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj as C
    rep = C.run()
    mine = {k["demangled"].split("(")[0].replace("void ", ""): k for k in rep["kernels"] if k["file"] == "skeleton.hip"}
    assert set(mine) >= {"soft_skel_fwd_kernel", "soft_skel_bwd_kernel", "cldice_finalize_kernel", "centerline_count_kernel"}
    for name, k in mine.items():
        assert k["hot"], name
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
