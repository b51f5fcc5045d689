"""Soft skeletons, the centerline loss clDice and the hard centerline metric on the device (csrc/skeleton.hip; trainer.soft_skeleton,
trainer.clDiceLoss, distance.centerline_counts, evaluate.centerline_metrics) against ``soft_skeleton_reference``, the numpy
restatement of the contract (tests/test_cldice_cpu.py holds it against torch autograd of the published formulation).

Exact cases (bit equality).  Quarter-valued inputs {0, 1/4, 1/2, 3/4, 1}: S_j needs 2 (j + 1) <= 22 fractional bits for iters <= 10, so
every fp32 operation of the forward is exact.  Binary inputs with small-integer upstream gradients: all arithmetic, forward and
backward, is integer, and what is tested is the tie rule (every min and max on a plateau ties).

Real-valued cases, against the reference in fp64 fed the same fp32 inputs (tie-free: distinct fp32 values, so the selections of
both precisions are the same).  With u = 2^-24:
  forward   |S - S64| <= 3 (iters + 1) u: three roundings per level (subtraction, fma, add) on values <= 1, propagated with the
            factor 1 - d <= 1.
  gradient  |g - g64| <= 4 (iters + 2) u A_i + 1e-30, A the reference's run with the absolute value of every routed term.  The
            kernels round twice per level in each of gd = gS (1 - S) and gS (1 - d), and once in each of the two routed sums (fp64
            gathers rounded once): a term born at level j has passed 2 (iters - j) + 2 roundings of factors and 2 (j + 1) of sums,
            2 (iters + 2) in all -- half of the bound ("Centerline loss (clDice)").
Loss, against an fp64 restatement built from the reference (``_cl64``), with the project's sigmoid / softplus gate 4e-6:
  value     |cl - cl64| <= 4 (4e-6 + 3 (iters + 1) u): two ratios of relative error e, harmonic mean <= 1.
  gradient  |dx - dx64| <= (4e-6 + 4 (iters + 2) u) (A_i + |b_i|) + 1e-30, A_i the absolute run of the skeleton path scaled by the
            coefficients and sigmoid', b_i the direct Sy part.
The logits of the loss cases are logit(tie-free p) rounded to fp32: neighbouring probabilities differ by more than 1e-5, so the
fp32 sigmoid of the device and the fp64 sigmoid of the restatement order them alike.  Needs a real MI355X."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _components_patterns as P
from conftest import record_margin
from hyperpri_amd import distance as D
from oracle import hyperpri_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
GATE = 4e-6


def _tile():
    from hyperpri_amd import _lib
    return int(_lib.load().hpri_soft_skeleton_tile())


@functools.lru_cache(maxsize=None)
def _shape(name):
    T = _tile()
    return {"5x3": (1, 1, 5, 3), "1x9": (1, 1, 1, 9), "9x1": (1, 1, 9, 1), "37x53": (3, 1, 37, 53),
            "ragged": (2, 1, 2 * T + 6, 3 * T + 3)}[name]       # ragged tiles both ways, the halo crosses tile and image borders


# (shape, iters): an image smaller than the halo; single rows and columns; several images; more than one tile; no erosion at all
CASES = [("5x3", 2), ("1x9", 3), ("9x1", 3), ("37x53", 5), ("ragged", 10), ("37x53", 0)]
IDS = [f"{n}-it{i}" for n, i in CASES]
# the deepest halo: more than 64 KB of LDS (the launcher has to ask for it), a halo as large as the image.  Not for the
# quarter-valued case: S_j would need 66 fractional bits.
DEEP = CASES + [("37x53", 32)]
DEEP_IDS = IDS + ["37x53-it32"]


# -- inputs (built once, never changed) ----------------------------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _tie_free(name, seed=3):
    shape = _shape(name)
    n = int(np.prod(shape))
    p = (0.02 + 0.96 * (np.random.RandomState(seed).permutation(n) + 1.0) / (n + 1)).astype(np.float32).reshape(shape)
    assert len(np.unique(p)) == n
    return _frozen(p)


def _bars(h, w):
    """Vertical bars of widths 1 .. 7 from the left border on, every other one stopping short of the top and bottom borders, and
    horizontal ones from the top border on that run into the right border: they cross the seams of every tile size and each other."""
    a = np.zeros((h, w), dtype=bool)
    x, k = 0, 0
    while x < w:
        wd = k % 7 + 1
        if k % 2 == 0:
            a[:, x:x + wd] = True
        else:
            a[2:max(h - 2, 3), x:x + wd] = True
        x += wd + 3
        k += 1
    y, k = 0, 3
    while y < h:
        wd = k % 7 + 1
        a[y:y + wd, w // 3:] = True
        y += wd + 5
        k += 1
    return a


@functools.lru_cache(maxsize=None)
def _binary(name):
    """Image 0: the bars; image 1: a full frame (N = 2) or an empty one (N = 3); image 2: a full frame."""
    N, _, h, w = _shape(name)
    a = np.zeros((N, 1, h, w), dtype=np.float32)
    a[0, 0] = _bars(h, w)
    if N >= 2:
        a[N - 1] = 1.0
    return _frozen(a)


@functools.lru_cache(maxsize=None)
def _roots(name):
    """A synthetic root mask (bars of three widths and a diagonal), blurred twice with a 3x3 box, made distinct by a small
    permutation ramp: plateaus of a saturated prediction turned into a tie-free plane."""
    N, _, h, w = _shape(name)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((N, h, w))
    for n in range(N):
        a = (np.abs(yy - h // 3 - n) < 1 + n) | (np.abs(xx - w // 4 - 2 * n) < 2) | (np.abs(yy * max(w, 2) - xx * max(h, 2)) < 2 * max(h, w))
        m[n] = a
    for _ in range(2):
        q = np.pad(m, ((0, 0), (1, 1), (1, 1)), mode="edge")
        m = sum(q[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    n_el = m.size
    ramp = 0.02 * np.random.RandomState(17).permutation(n_el).reshape(m.shape) / n_el
    p = (0.03 + 0.9 * m + ramp).astype(np.float32).reshape(_shape(name))
    assert len(np.unique(p)) == n_el and p.min() >= 0 and p.max() <= 1
    return _frozen(p)


@functools.lru_cache(maxsize=None)
def _upstream(name, integer=False):
    rng = np.random.RandomState(23)
    g = rng.randint(-3, 4, size=_shape(name)).astype(np.float32) if integer else rng.uniform(-1, 1, size=_shape(name)).astype(np.float32)
    return _frozen(g)


@functools.lru_cache(maxsize=None)
def _ref(kind, name, iters, with_grad=True):
    """The reference's answer for an input, computed once per session."""
    p = {"tie_free": _tie_free, "roots": _roots, "binary": _binary}[kind](name)
    if not with_grad:
        return soft_ref(p, iters)
    g = _upstream(name, integer=kind == "binary")
    return soft_ref(p, iters, g)


def soft_ref(p32, iters, g32=None):
    if g32 is None:
        return D.soft_skeleton_reference(p32.astype(np.float64), iters)
    return D.soft_skeleton_reference(p32.astype(np.float64), iters, grad=g32.astype(np.float64))


def _dev(p32, iters, g32=None, tensor=None):
    import hyperpri_amd as H
    t = (torch.from_numpy(np.array(p32)).to(DEV) if tensor is None else tensor).requires_grad_(g32 is not None)
    S = H.soft_skeleton(t, iters)
    assert S.shape == t.shape and S.dtype == torch.float32
    if g32 is None:
        return S.cpu().numpy(), None
    S.backward(torch.from_numpy(np.array(g32)).to(DEV))
    return S.detach().cpu().numpy(), t.grad.cpu().numpy()


# -- exact cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,iters", CASES, ids=IDS)
def test_forward_is_exact_on_quarter_valued_inputs(name, iters):
    p = (np.random.RandomState(41).randint(0, 5, size=_shape(name)) / 4.0).astype(np.float32)
    S, _ = _dev(p, iters)
    want = soft_ref(p, iters)
    assert np.array_equal(S.astype(np.float64), want)
    assert iters == 0 or name == "5x3" or want.max() > 0


@pytest.mark.parametrize("name,iters", DEEP, ids=DEEP_IDS)
def test_forward_and_gradient_are_exact_on_binary_inputs(name, iters):
    """Plateaus everywhere: the first-optimum rule decides every route."""
    p, g = _binary(name), _upstream(name, integer=True)
    S, gp = _dev(p, iters, g)
    wS, wg, _ = _ref("binary", name, iters)
    assert np.array_equal(S.astype(np.float64), wS)
    assert np.array_equal(gp.astype(np.float64), wg)
    assert set(np.unique(wS)) <= {0.0, 1.0} and (name not in ("37x53", "ragged") or np.abs(wg).max() > 0)


def test_two_runs_give_identical_bytes():
    import hyperpri_amd as H
    p, g = _roots("ragged"), _upstream("ragged")
    a, b = _dev(p, 10, g), _dev(p, 10, g)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    x, y = _loss_inputs("37x53")
    for per_image in (False, True):
        r1, r2 = _run_loss(x, y, H.clDiceLoss(iters=5, per_image=per_image), 0.37), _run_loss(x, y, H.clDiceLoss(iters=5, per_image=per_image), 0.37)
        assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and torch.equal(r1[2], r2[2])


def test_a_misaligned_view_gives_the_bytes_of_its_contiguous_copy():
    import hyperpri_amd as H
    name, iters = "37x53", 5
    p, g = _roots(name), _upstream(name)
    buf = torch.empty(p.size + 8, dtype=torch.float32, device=DEV)
    view = buf[1:1 + p.size].view(p.shape)
    view.copy_(torch.from_numpy(np.array(p)))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    a, b = _dev(p, iters, g), _dev(p, iters, g, tensor=view.detach())
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    x, y = _loss_inputs(name)
    xbuf = torch.empty(x.numel() + 8, dtype=torch.float32, device=DEV)
    xview = xbuf[3:3 + x.numel()].view(x.shape)
    xview.copy_(x)
    r1, r2 = _run_loss(x, y, H.clDiceLoss(iters=iters), 1.0), _run_loss(x, y, H.clDiceLoss(iters=iters), 1.0, x_dev=xview.detach())
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


# -- real-valued cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tie_free", "roots"])
@pytest.mark.parametrize("name,iters", DEEP, ids=DEEP_IDS)
def test_forward_and_gradient_stay_within_the_derived_bounds(name, iters, kind):
    p = {"tie_free": _tie_free, "roots": _roots}[kind](name)
    g = _upstream(name)
    S, gp = _dev(p, iters, g)
    S64, g64, A = _ref(kind, name, iters)
    ferr, ftol = float(np.abs(S - S64).max()), 3 * (iters + 1) * U
    tol = 4 * (iters + 2) * U * A + 1e-30
    ratio = float((np.abs(gp - g64) / tol).max())
    print(f"{kind} {name} iters {iters}: forward {ferr / U:.2f} u of {ftol / U:.0f} u; gradient {ratio:.3f} of its bound; max A {A.max():.2e}")
    record_margin(f"cldice/skeleton_fwd/{kind}/{name}/it{iters}", ferr, ftol)
    record_margin(f"cldice/skeleton_bwd/{kind}/{name}/it{iters}", ratio, 1.0)
    assert ferr <= ftol
    assert ratio <= 1.0
    assert A.max() > 0 and (name in ("1x9", "9x1", "5x3") or S64.max() > 0.01)


# -- the loss ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_inputs(name):
    """Logits = logit(tie-free p) in fp32 with +-40 planted on both target values (far from each other); the target: the bars."""
    N, _, h, w = _shape(name)
    p = _tie_free(name, seed=5).astype(np.float64)
    x = np.log(p / (1 - p)).astype(np.float32)
    y = np.zeros(_shape(name), dtype=np.float32)
    for n in range(N):
        y[n, 0] = _bars(h, w) if n % 2 == 0 else _bars(w, h).T
    xf, yf = x.reshape(-1), y.reshape(-1)
    n_el = xf.size
    for i, (xv, yv) in zip((1, n_el // 4, n_el // 2, n_el - 2), ((40.0, 1.0), (-40.0, 1.0), (40.0, 0.0), (-40.0, 0.0))):
        xf[i], yf[i] = xv, yv
    return torch.from_numpy(x), torch.from_numpy(y)


def _sig64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


@functools.lru_cache(maxsize=None)
def _cl64_cached(name, iters, s, per_image):
    x, y = _loss_inputs(name)
    return _cl64(x.numpy().astype(np.float64), y.numpy().astype(np.float64), iters, s, per_image)


def _cl64(x, y, iters, s, per_image):
    """The centerline term in fp64 from the reference: (cl, dcl/dx, A, b) with the edge rules of the contract (a ratio with a zero
    denominator is 0; tprec + tsens == 0 gives cl = 1 and a zero gradient).  A: the absolute run of the skeleton path scaled by
    sigmoid'; b: the direct Sy part."""
    sp, sn = _sig64(x), _sig64(-x)
    planes = x.reshape((-1,) + x.shape[-2:])
    yp, pp = y.reshape(planes.shape), sp.reshape(planes.shape)
    Sp, Sy = D.soft_skeleton_reference(pp, iters), D.soft_skeleton_reference(yp, iters)
    groups = [[n] for n in range(len(planes))] if per_image else [list(range(len(planes)))]
    gSp, c = np.zeros_like(pp), np.zeros_like(pp)
    cl = 0.0
    for idx in groups:
        a1, a2, b1, b2 = (Sp[idx] * yp[idx]).sum(), Sp[idx].sum(), (Sy[idx] * pp[idx]).sum(), Sy[idx].sum()
        tp = (a1 + s) / (a2 + s) if a2 + s != 0 else 0.0
        ts = (b1 + s) / (b2 + s) if b2 + s != 0 else 0.0
        if tp + ts == 0:
            cl += 1.0
            continue
        cl += 1 - 2 * tp * ts / (tp + ts)
        k = 1.0 / len(groups)
        dtp, dts = -2 * ts * ts / (tp + ts) ** 2, -2 * tp * tp / (tp + ts) ** 2
        if a2 + s != 0:
            gSp[idx] = k * dtp * (yp[idx] / (a2 + s) - (a1 + s) / (a2 + s) ** 2)
        if b2 + s != 0:
            c[idx] = k * dts / (b2 + s)
    _, gp, A = D.soft_skeleton_reference(pp, iters, grad=gSp)
    d = (sp * sn).reshape(planes.shape)
    direct = c * Sy
    return cl / len(groups), ((gp + direct) * d).reshape(x.shape), (A * d).reshape(x.shape), np.abs(direct * d).reshape(x.shape)


def _run_loss(x, y, crit, g, x_dev=None):
    xg = (x.to(DEV) if x_dev is None else x_dev).requires_grad_(True)
    loss = crit(xg, y.to(DEV))
    (loss * g).backward()
    return loss.detach(), xg.grad, crit.last_terms


@pytest.mark.parametrize("s", [0.0, 1.0])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("name,iters", [("5x3", 2), ("37x53", 5), ("ragged", 10), ("37x53", 0), ("37x53", 32)])
def test_the_centerline_term_matches_its_fp64_restatement(name, iters, per_image, s):
    import hyperpri_amd as H
    x, y = _loss_inputs(name)
    g = 0.37
    loss, dx, terms = _run_loss(x, y, H.clDiceLoss(iters=iters, alpha=1.0, smooth=s, per_image=per_image), g)
    cl64, dx64, A, b = _cl64_cached(name, iters, s, per_image)
    verr, vtol = abs(float(loss) - cl64), 4 * (GATE + 3 * (iters + 1) * U)
    tol = (GATE + 4 * (iters + 2) * U) * abs(g) * (A + b) + 1e-30
    ratio = float((np.abs(dx.cpu().numpy() - g * dx64) / tol).max())
    print(f"cl {name} iters {iters} per_image {per_image} s {s}: value {float(loss)!r} (fp64 {cl64!r}) error {verr:.2e} of {vtol:.2e}; "
          f"gradient {ratio:.3f} of its bound")
    record_margin(f"cldice/loss/{name}/it{iters}/img{int(per_image)}/s{s}", verr, vtol)
    record_margin(f"cldice/loss_grad/{name}/it{iters}/img{int(per_image)}/s{s}", ratio, 1.0)
    assert verr <= vtol
    assert ratio <= 1.0
    assert float(terms[0]) == pytest.approx(cl64, abs=vtol) and 0 < cl64 < 1 and np.abs(dx64).max() > 0
    assert bool(torch.isfinite(dx).all())


def test_the_weighted_sum_with_a_base_and_the_alpha_ends():
    """(1 - alpha) base + alpha cl: the value to fp32 rounding of the two terms' own values, the gradient as the sum of the two
    terms' own gradients scaled (the base's backward reads its upstream gradient from the device); alpha = 0 is the base bit for bit."""
    import hyperpri_amd as H
    x, y = _loss_inputs("37x53")
    lb, gb, _ = _run_loss(x, y, H.DiceBCELoss(pos_weight=3.0), 1.0)
    lc, gc, _ = _run_loss(x, y, H.clDiceLoss(iters=3, alpha=1.0), 1.0)
    l0, g0, _ = _run_loss(x, y, H.clDiceLoss(iters=3, alpha=0.0, base=H.DiceBCELoss(pos_weight=3.0)), 1.0)
    assert torch.equal(l0, lb) and torch.equal(g0, gb)
    lm, gm, _ = _run_loss(x, y, H.clDiceLoss(iters=3, alpha=0.25, base=H.DiceBCELoss(pos_weight=3.0)), 1.0)
    want = 0.75 * float(lb) + 0.25 * float(lc)
    assert abs(float(lm) - want) <= 2 * U * abs(want)
    wg = 0.75 * gb.double() + 0.25 * gc.double()
    scale = 0.75 * gb.double().abs() + 0.25 * gc.double().abs()
    assert bool(((gm.double() - wg).abs() <= 4 * U * scale + 1e-30).all())
    ld, gd, _ = _run_loss(x, y, H.clDiceLoss(iters=3), 1.0)                     # the default base: DiceLoss(smooth)
    lD, _, _ = _run_loss(x, y, H.DiceLoss(1.0), 1.0)
    assert abs(float(ld) - (0.5 * float(lD) + 0.5 * float(lc))) <= 2 * U


def test_edge_rules_shapes_and_dtypes():
    import hyperpri_amd as H
    x, y = _loss_inputs("37x53")
    xd, yd = x.to(DEV), y.to(DEV)
    crit = H.clDiceLoss(iters=3)
    base = crit(xd, yd)
    for form in (yd.to(torch.uint8), yd.double(), yd.bool()):
        assert torch.equal(crit(xd, form), base), form.dtype
    with pytest.raises(ValueError, match="must be the same as input size"):
        crit(xd, yd[:, 0])
    # an empty target without smoothing: Sy = 0, tsens = 0 / 0 -> 0; Sp * y = 0 -> tprec = 0: cl = 1, no gradient
    loss, dx, terms = _run_loss(x, torch.zeros_like(y), H.clDiceLoss(iters=3, alpha=1.0, smooth=0.0, per_image=True), 1.0)
    assert float(loss) == 1.0 and not bool(dx.any()) and terms.tolist() == [1.0, 0.0, 0.0]
    # the same target with smoothing: finite, and a gradient
    loss, dx, _ = _run_loss(x, torch.zeros_like(y), H.clDiceLoss(iters=3, alpha=1.0, smooth=1.0), 1.0)
    assert 0 <= float(loss) <= 1 and bool(torch.isfinite(dx).all()) and bool(dx.any())
    # soft_skeleton without a gradient keeps nothing and agrees with the run that does
    p = torch.from_numpy(np.array(_roots("37x53"))).to(DEV)
    with torch.no_grad():
        a = H.soft_skeleton(p, 5)
    assert not a.requires_grad and torch.equal(a, H.soft_skeleton(p.clone().requires_grad_(True), 5).detach())
    assert torch.equal(H.soft_skeleton(p[:, 0], 5), a[:, 0])                   # (N, h, w) planes
    with pytest.raises(RuntimeError, match="float32"):
        H.soft_skeleton(p.double(), 2)


# -- one training step ---------------------------------------------------------------------------------------------------------------
def _u(seed, shape):
    return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())


def _loss64(l64, m64, iters):
    """0.5 Dice(smooth 1, batch) + 0.5 cl(iters, smooth 1, batch) in fp64: (value, d/dlogits)."""
    x = l64.clone().requires_grad_(True)
    p = torch.exp(-torch.nn.functional.softplus(-x))
    inter = (p * m64).sum()
    dice = 1 - (2 * inter + 1) / (p.sum() + m64.sum() + 1)
    dice.backward()
    cl, dcl, _, _ = _cl64(l64.numpy(), m64.numpy(), iters, 1.0, False)
    return 0.5 * float(dice.detach()) + 0.5 * cl, 0.5 * x.grad + 0.5 * torch.from_numpy(dcl)


def _oracle_step(sd, x, m, dtype):
    leaves, work = OrderedDict(), OrderedDict()
    for k, v in sd.items():
        if O.is_param(k):
            leaves[k] = work[k] = v.detach().to(dtype).clone().requires_grad_(True)
        else:
            work[k] = v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()
    logits = O.unet_forward(work, x.to(dtype))
    value, dl = _loss64(logits.detach().double(), m.double(), 3)
    logits.backward(dl.to(dtype))
    return logits.detach(), value, OrderedDict((k, p.grad) for k, p in leaves.items())


def test_unet3_one_step_under_cldice_matches_the_cpu_oracle(monkeypatch):
    """UNet(3, 1) at (2, 3, 36, 50) in fp32, one training_step of SegmentationModel(net, clDiceLoss(iters=3)) against the fp32 CPU
    oracle fed with the fp64 dlogits of the restated loss, with the tolerances of
    test_gpu_segloss.py::test_unet3_one_step_under_dice_bce_matches_the_cpu_oracle: logits 1e-3, loss 1e-5, gradients 2e-3 in relative
    L2 of the difference; convolution biases in front of a train-mode BatchNorm (true gradient 0) are skipped.  The target is a drawn
    root mask, so that it has a skeleton."""
    import hyperpri_amd as H
    from hyperpri_amd import trainer as T
    sd = O.synth_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in H.UNet(3, 1, bilinear=False).state_dict().items()))
    x = _u(1234, (2, 3, 36, 50))
    m = torch.from_numpy(np.stack([_bars(36, 50), _bars(50, 36).T]).astype(np.float32)).view(2, 1, 36, 50)
    ref_logits, ref_loss, ref_grads = _oracle_step(sd, x, m, torch.float32)
    _, _, grads64 = _oracle_step(sd, x, m, torch.float64)
    taken = []
    real = T.forward_loss
    monkeypatch.setattr(T, "forward_loss", lambda *a, **k: (taken.append(1), real(*a, **k))[1])
    net = H.UNet(3, 1, bilinear=False)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    model = H.SegmentationModel(net, H.clDiceLoss(iters=3))
    logits, loss = model._step("tr", {"image": x.to(DEV), "mask": m.to(DEV)}, model.threshold)
    loss.backward()
    assert not taken and type(loss.grad_fn).__name__.startswith("_clDiceFn")
    err = float((logits.detach().cpu() - ref_logits).abs().max())
    print(f"unet3 under clDice: max|dlogit| {err:.2e}, loss {float(loss.detach())!r} (oracle {ref_loss!r})")
    assert err < 1e-3
    assert abs(float(loss.detach()) - ref_loss) < 1e-5
    grads = dict(net.named_parameters())
    checked = 0
    for k, ref in ref_grads.items():
        g64 = grads64[k]
        if float(g64.norm()) < 1e-12:
            assert k.endswith(".bias")
            continue
        got = grads[k].grad.detach().cpu().double()
        rel = float((got - ref.double()).norm() / ref.double().norm())
        print(f"  {k}: relative L2 {rel:.2e} (oracle fp32-fp64 spread {float((ref.double() - g64).norm() / g64.norm()):.2e})")
        assert rel <= 2e-3, (k, rel)
        checked += 1
    assert checked >= 55


# -- the hard metric -----------------------------------------------------------------------------------------------------------------
METRIC_SHAPE = (P.TILE_H + 5, 2 * P.TILE_W - 7)
METRIC_NAMES = ("empty", "full", "checkerboard", "spiral", "comb", "diagonal", "stripes_both", "noise_0.41", "noise_0.8")


@functools.lru_cache(maxsize=None)
def _thin(name):
    return D.thin_reference(P.pattern(name, METRIC_SHAPE)).astype(bool)


def _want_counts(pred, truth, sp, st):
    return np.stack([sp.sum(axis=(1, 2)), (sp & truth).sum(axis=(1, 2)), st.sum(axis=(1, 2)), (st & pred).sum(axis=(1, 2))], axis=1).astype(np.int64)


@pytest.mark.parametrize("k", range(len(METRIC_NAMES)))
def test_centerline_counts_are_exact_against_the_thinning_reference(k):
    """Pattern k as the prediction against pattern k + 1 as the truth (cyclic): an empty prediction at k = 0, an empty truth at the
    last k."""
    pn, tn = METRIC_NAMES[k], METRIC_NAMES[(k + 1) % len(METRIC_NAMES)]
    pred, truth = P.pattern(pn, METRIC_SHAPE), P.pattern(tn, METRIC_SHAPE)
    want = _want_counts(pred, truth, _thin(pn), _thin(tn))
    dp = torch.from_numpy(np.ascontiguousarray(pred).astype(np.uint8)).to(DEV)
    dt = torch.from_numpy(np.ascontiguousarray(truth).astype(np.float32)).to(DEV)
    got = D.centerline_counts(dp, None, dt)
    assert got.dtype == np.int64 and np.array_equal(got, want), (pn, tn)
    m, ref = D.centerline_metrics(dp, None, dt), D.centerline_from_counts(want)
    for key in ("tprec", "tsens", "cldice"):
        assert np.array_equal(m[key], ref[key], equal_nan=True) and (m["pooled"][key] == ref["pooled"][key] or np.isnan(ref["pooled"][key]))
    if pn == "empty":
        assert np.isnan(m["tprec"]).all() and (m["tsens"] == 0).all() and np.isnan(m["cldice"]).all()
    if tn == "empty":
        assert np.isnan(m["tsens"]).all() and (m["tprec"] == 0).all()


def test_centerline_metrics_over_a_split_pool_the_per_image_counts():
    import hyperpri_amd as H
    thr = 0.35
    sizes = [METRIC_SHAPE] * 3 + [(20, 33)] * 2
    maps = [(P.pattern("noise_0.8", METRIC_SHAPE)[i], P.pattern("stripes_both", METRIC_SHAPE)[i]) for i in range(3)]
    maps += [(P.pattern("comb", (20, 33))[i], P.pattern("noise_0.8", (20, 33))[i]) for i in range(2)]
    offsets = [0]
    for h, w in sizes:
        offsets.append(offsets[-1] + h * w)
    logits, masks = torch.empty(offsets[-1]), torch.empty(offsets[-1])
    rng = np.random.RandomState(9)
    for i, (a, t) in enumerate(maps):
        u = torch.from_numpy(rng.rand(*a.shape).astype(np.float32))
        centre = float(np.log(thr / (1 - thr)))
        logits[offsets[i]:offsets[i + 1]] = (centre + torch.where(torch.from_numpy(np.array(a)), 0.1 + 3 * u, -(0.1 + 3 * u))).reshape(-1)
        masks[offsets[i]:offsets[i + 1]] = torch.from_numpy(np.array(t).astype(np.float32).reshape(-1))
    split = H.SplitPrediction(logits.to(DEV), masks.to(DEV), offsets, sizes, [f"img{i}" for i in range(5)])
    got = H.centerline_metrics(split, thr)
    want = np.concatenate([_want_counts(a[None], t[None], D.thin_reference(a).astype(bool)[None], D.thin_reference(t).astype(bool)[None])
                           for a, t in maps])
    ref = D.centerline_from_counts(want)
    assert got["per_image"]["counts"] == want.tolist() and got["names"] == split.names
    for key in ("tprec", "tsens", "cldice"):
        assert got[key] == ref["pooled"][key] and 0 < got[key] < 1
        assert np.array_equal(np.asarray(got["per_image"][key]), ref[key], equal_nan=True)
