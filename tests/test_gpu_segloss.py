"""The imbalance-aware binary losses on the device (csrc/segloss.hip; trainer.SegLoss, DiceLoss, TverskyLoss, FocalLoss, DiceBCELoss,
BCEWithLogitsLoss(pos_weight, reduction)) against an fp64 restatement of the family on the CPU, written with softplus and
sigmoid(-x) and differentiated by torch autograd:

    loss = w_point * R[ a_t * (1 - p_t)^gf * ce ] + w_overlap * mean_groups[ (1 - T_g)^gt ]
    ce = pos_weight * y * softplus(-x) + (1 - y) * softplus(x),   1 - p_t = y * sigmoid(-x) + (1 - y) * sigmoid(x)
    T_g = (I + s) / (I + alpha (P - I) + beta (Y - I) + s),   I = sum p y, P = sum p, Y = sum y

The reference's sigmoid is exp(-softplus(-x)): autograd's own sigmoid backward, s * (1 - s), is 0 at x = 40 in fp64 where the true
derivative is 4e-18.

Gates.  Loss: 1e-6 relative (the project's BCE / CE gate).  Gradients, per element: |dx - dx64| <= rtol * (|a_i| + |b_i|) + 1e-30 with
a and b the reference's pointwise and overlap parts (two autograd calls; the parts may cancel, so a bound relative to their sum could
not be met) and rtol = 4e-6, the cross-entropy gate of test_gpu_multiclass.py: |x| <= 8 rounds the exponent at 4.8e-7, expf, the
division, log1pf and powf add about an ulp each, the products another few, the total doubled.  The same closed form evaluated in fp32
torch on the CPU in the sigmoid(-x) form (``_closed_form32`` below; asserted in tests/test_segloss_cpu.py, which runs without a GPU) stays within 0.17 of that allowance for the focal cases (gamma 2
with alpha 0.25: 0.164; gamma 1.5 with pos_weight 2: 0.154; worst element over the four shapes, the other configurations 0.03 to
0.11), so twice its error is inside rtol = 4e-6 and the focal cases keep that rtol.  The 1e-30 covers values below fp32's normal
range only: the planted confident pixels' focal gradients fall to 1e-57.

Soft labels.  With a uniform soft label the gradient has zeros of its own inside the input range -- the pointwise part at
sigmoid(x) = y for plain BCE, the overlap part at c1 * y + c0 = 0 -- where no fp32 evaluation of a sigmoid keeps accuracy relative
to the result (the fp32 closed form on the CPU misses the gate above by factors of 2.6 to 12 at (3, 1, 37, 53)).  So the soft-label
case under the gate above is the overlap losses on label-smoothed targets, whose conditioning the test checks on the reference, and
``test_soft_labels_gradient_of_the_terms`` holds uniform soft labels to rtol times the sum of the MAGNITUDES of the terms the closed
form adds (the forward error bound of a sum; the fp32 closed form on the CPU: 0.05 to 0.12 of it).  Needs a real MI355X."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import hyperpri_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 4e-6


def _u(seed, shape):
    return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())


def _ragged_shape():
    """(2, hw) with hw = 2 sweeps of every block of an image + 5: the blocks-per-image cap comes from the library's own constants."""
    from hyperpri_amd import _lib
    cap = _lib.load().hpri_seg_loss_workspace_doubles(2, 1 << 40) // (4 * 2)
    return (2, 2 * cap * 1024 + 5)


SHAPES = {
    "3x1x37x53": (3, 1, 37, 53),       # hw = 1961: images 1 and 2 start misaligned, element accesses, a short last quad
    "2x1x16x24": (2, 1, 16, 24),       # 16-byte accesses, less than one block per image
    "1x1x5x3": (1, 1, 5, 3),           # fewer elements than lanes
    "ragged": None,                    # every block of an image wraps its stride loop, ragged tail (filled in lazily)
}


def _shape(name):
    return SHAPES[name] or _ragged_shape()


@functools.lru_cache(maxsize=None)
def _inputs(name, soft=False):
    """Logits in [-8, 8) with +-40 planted on both target values; hard targets with about 8 % positives.  soft = "smooth": those
    targets label-smoothed to 0.05 / 0.95; soft = "uniform": targets uniform in [0, 1)."""
    shape = _shape(name)
    x = _u(301, shape) * 16 - 8
    y = (_u(302, shape) > 0.92).float()
    xf, yf = x.view(-1), y.view(-1)
    n = xf.numel()
    for i, (xv, yv) in zip((1, 2, n - 1, n // 2), ((40.0, 1.0), (-40.0, 1.0), (40.0, 0.0), (-40.0, 0.0))):
        xf[i], yf[i] = xv, yv
    if soft == "smooth":
        y = 0.05 + 0.9 * y
    elif soft == "uniform":
        y = _u(303, shape)
    return x, y


# name: (criterion factory, the family's parameters as the reference takes them, upstream gradient)
def _P(wp=1.0, pw=1.0, gf=0.0, af=None, mean=True, wo=0.0, al=0.5, be=0.5, s=0.0, gt=1.0, per_image=False):
    return dict(wp=wp, pw=pw, gf=gf, af=af, mean=mean, wo=wo, al=al, be=be, s=s, gt=gt, per_image=per_image)


CONFIGS = OrderedDict([
    ("wbce", (lambda H: H.BCEWithLogitsLoss(pos_weight=3.0), _P(pw=3.0), 1.0)),
    ("wbce_sum", (lambda H: H.BCEWithLogitsLoss(pos_weight=torch.tensor([3.0]), reduction="sum"), _P(pw=3.0, mean=False), 0.37)),
    ("focal", (lambda H: H.FocalLoss(gamma=2.0, alpha=0.25), _P(gf=2.0, af=0.25), 1.0)),
    ("focal15_pw", (lambda H: H.SegLoss(focal_gamma=1.5, pos_weight=2.0), _P(gf=1.5, pw=2.0), 2.5)),
    ("dice_batch", (lambda H: H.DiceLoss(smooth=1.0), _P(wp=0.0, wo=1.0, s=0.5), 1.0)),      # (2I + 1) / (P + Y + 1)
    ("tversky_img", (lambda H: H.TverskyLoss(0.3, 0.7, 1.0, per_image=True), _P(wp=0.0, wo=1.0, al=0.3, be=0.7, s=1.0, per_image=True), 0.37)),
    ("focal_tversky_img", (lambda H: H.TverskyLoss(0.3, 0.7, 1.0, gamma=0.75, per_image=True),
                           _P(wp=0.0, wo=1.0, al=0.3, be=0.7, s=1.0, gt=0.75, per_image=True), 1.0)),
    ("dicebce", (lambda H: H.DiceBCELoss(1.0, 0.5, pos_weight=3.0), _P(pw=3.0, wo=0.5, s=0.5), 1.0)),
])


def _softplus(z):
    return torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))


def _sig(z):
    return torch.exp(-_softplus(-z))


def _family(x, y, p):
    """(weighted pointwise term, weighted overlap term, mean T) of the family in the dtype of x, differentiable."""
    zero = x.sum() * 0
    point, over, mean_t = zero, zero, zero
    if p["wp"] != 0:
        v = p["pw"] * y * _softplus(-x) + (1 - y) * _softplus(x)
        if p["gf"] != 0:
            v = v * (y * _sig(-x) + (1 - y) * _sig(x)) ** p["gf"]
        if p["af"] is not None:
            v = v * (p["af"] * y + (1 - p["af"]) * (1 - y))
        point = p["wp"] * (v.mean() if p["mean"] else v.sum())
    if p["wo"] != 0:
        rows = x.shape[0] if p["per_image"] else 1
        pr, yr = _sig(x).reshape(rows, -1), y.reshape(rows, -1)
        i_, p_, y_ = (pr * yr).sum(1), pr.sum(1), yr.sum(1)
        t = (i_ + p["s"]) / (i_ + p["al"] * (p_ - i_) + p["be"] * (y_ - i_) + p["s"])
        over = p["wo"] * ((1 - t) ** p["gt"]).mean()
        mean_t = t.mean()
    return point, over, mean_t


@functools.lru_cache(maxsize=None)
def _reference(name, config, soft=False):
    """fp64: (loss, pointwise term, overlap term, mean T, a, b) with a, b the two parts of g * dloss/dx; computed once per case."""
    _, p, g = CONFIGS[config]
    x, y = _inputs(name, soft)
    xd = x.double().requires_grad_(True)
    point, over, mean_t = _family(xd, y.double(), p)
    a = torch.autograd.grad(point * g, xd, retain_graph=True)[0] if p["wp"] != 0 else torch.zeros_like(xd)
    b = torch.autograd.grad(over * g, xd)[0] if p["wo"] != 0 else torch.zeros_like(xd)
    return float((point + over).detach()), float(point.detach()), float(over.detach()), float(mean_t.detach()), a, b


def _closed_form32(x, y, p, g):
    """The kernels' closed form in fp32 torch on the CPU (sigmoid(x), sigmoid(-x) and log1p from one exp(-|x|); 1 - p_t direct; the
    group sums and coefficients in fp64): what fp32 arithmetic gives for dx, independent of the HIP code."""
    e = torch.exp(-x.abs())
    r = 1 / (1 + e)
    sp, sn, lg = torch.where(x >= 0, r, e * r), torch.where(x >= 0, e * r, r), torch.log1p(e)
    dx = torch.zeros_like(x)
    if p["wp"] != 0:
        d = (1 - y) * sp - p["pw"] * y * sn
        if p["gf"] != 0 or p["af"] is not None:
            q = y * sn + (1 - y) * sp
            ce = p["pw"] * y * (torch.clamp(-x, min=0) + lg) + (1 - y) * (torch.clamp(x, min=0) + lg)
            ratio = torch.where(q > 0, sp * sn / q, torch.zeros_like(q))
            at = 1.0 if p["af"] is None else p["af"] * y + (1 - p["af"]) * (1 - y)
            d = at * q ** p["gf"] * (p["gf"] * (1 - 2 * y) * ratio * ce + d)
        dx = d * np.float32(p["wp"] / x.numel() if p["mean"] else p["wp"])
    if p["wo"] != 0:
        rows = x.shape[0] if p["per_image"] else 1
        pr, yr = sp.double().reshape(rows, -1), y.double().reshape(rows, -1)
        i_, p_, y_ = (pr * yr).sum(1), pr.sum(1), yr.sum(1)
        num = i_ + p["s"]
        den = i_ + p["al"] * (p_ - i_) + p["be"] * (y_ - i_) + p["s"]
        dldt = -p["gt"] * (1 - num / den) ** (p["gt"] - 1)
        k = p["wo"] / rows * dldt / den ** 2
        c1, c0 = k * (den - num * (1 - p["al"] - p["be"])), k * (-num * p["al"])
        coef = (c1[:, None] * yr + c0[:, None]).float().reshape(x.shape)
        dx = dx + coef * (sp * sn)
    return dx * np.float32(g)


def _run(name, config, soft=False, x_dev=None):
    """(loss, dlogits, the criterion) of one case on the device."""
    import hyperpri_amd as H
    make, _, g = CONFIGS[config]
    x, y = _inputs(name, soft)
    xg = (x.to(DEV) if x_dev is None else x_dev).detach().requires_grad_(True)
    crit = make(H).to(DEV)
    loss = crit(xg, y.to(DEV))
    assert loss.shape == () and loss.dtype == torch.float32
    (loss * g).backward()
    return loss.detach(), xg.grad, crit


def _check(name, config, soft=False):
    ref_loss, ref_point, ref_over, ref_t, a, b = _reference(name, config, soft)
    loss, grad, crit = _run(name, config, soft)
    got = float(loss)
    rel = abs(got - ref_loss) / abs(ref_loss)
    allow = RTOL * (a.abs() + b.abs()) + 1e-30
    err = (grad.double().cpu() - (a + b)).abs()
    worst = float((err / allow).max())
    print(f"seg loss {name} {config}{' soft' if soft else ''}: loss {got!r} (fp64 {ref_loss!r}, rel {rel:.2e}); "
          f"gradient error / allowance {worst:.3f}")
    assert rel <= 1e-6
    assert worst <= 1.0
    seg = getattr(crit, "_seg", crit)
    terms = seg.last_terms.cpu().double()
    _, p, _ = CONFIGS[config]
    for k, (want, weight) in enumerate(((ref_point, p["wp"]), (ref_over, p["wo"]))):
        if weight != 0:
            assert abs(float(terms[k]) * weight - want) <= 1e-6 * abs(want), (k, float(terms[k]), want)
        else:
            assert float(terms[k]) == 0.0
    if p["wo"] != 0:
        assert abs(float(terms[2]) - ref_t) <= 1e-6 * abs(ref_t)
    return loss, grad


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_seg_losses_match_the_fp64_family(name, config):
    loss, grad = _check(name, config)
    x, y = _inputs(name)
    n = x.numel()
    if CONFIGS[config][1]["wp"] != 0 and CONFIGS[config][1]["wo"] == 0:
        # the planted confident pixels: a wrong one pulls hard, a right one keeps the sign of its tiny gradient (or underflows to 0)
        gf = grad.view(-1).cpu()
        assert float(gf[2]) < 0.0 and float(gf[n - 1]) > 0.0 and float(gf[1]) <= 0.0 and float(gf[n // 2]) >= 0.0


def _coefficients(x, y, p):
    """fp64: the groups' backward coefficients (c1, c0) of the closed form, broadcast to the elements."""
    rows = x.shape[0] if p["per_image"] else 1
    pr, yr = _sig(x).reshape(rows, -1), y.reshape(rows, -1)
    i_, p_, y_ = (pr * yr).sum(1), pr.sum(1), yr.sum(1)
    num = i_ + p["s"]
    den = i_ + p["al"] * (p_ - i_) + p["be"] * (y_ - i_) + p["s"]
    k = p["wo"] / rows * (-p["gt"] * (1 - num / den) ** (p["gt"] - 1)) / den ** 2
    c1, c0 = k * (den - num * (1 - p["al"] - p["be"])), k * (-num * p["al"])
    return (c1[:, None] * torch.ones_like(yr)).reshape(x.shape), (c0[:, None] * torch.ones_like(yr)).reshape(x.shape)


def _magnitudes(x, y, p, g):
    """fp64: per element, the sum of the magnitudes of the terms the closed form adds up to dx (the forward error bound of a sum)."""
    sp, sn = _sig(x), _sig(-x)
    mag = torch.zeros_like(x)
    if p["wp"] != 0:
        q = y * sn + (1 - y) * sp
        ce = p["pw"] * y * _softplus(-x) + (1 - y) * _softplus(x)
        at = 1.0 if p["af"] is None else p["af"] * y + (1 - p["af"]) * (1 - y)
        mag = p["wp"] / (x.numel() if p["mean"] else 1) * at * q ** p["gf"] * (p["gf"] * (1 - 2 * y).abs() * (sp * sn / q) * ce
                                                                          + p["pw"] * y * sn + (1 - y) * sp)
    if p["wo"] != 0:
        c1, c0 = _coefficients(x, y, p)
        mag = mag + (c1.abs() * y + c0.abs()) * sp * sn
    return abs(g) * mag


@pytest.mark.parametrize("config", ["dice_batch", "tversky_img"])
@pytest.mark.parametrize("name", ["3x1x37x53", "2x1x16x24"])
def test_soft_labels_soft_dice(name, config):
    """The soft-label case under the gate of the hard-label cases: label-smoothed targets (0.05 / 0.95) under the overlap losses.
    Its precondition is checked on the fp64 reference: c1 * y + c0 keeps more than an eighth of |c1| y + |c0| at every element, so
    the gate's |b_i| is of the size of what fp32 adds up (uniform soft labels: test_soft_labels_gradient_of_the_terms)."""
    _, p, g = CONFIGS[config]
    x, y = (t.double() for t in _inputs(name, "smooth"))
    c1, c0 = _coefficients(x, y, p)
    assert bool(((c1 * y + c0).abs() * 8 >= c1.abs() * y + c0.abs()).all())
    _check(name, config, soft="smooth")


@pytest.mark.parametrize("config", ["wbce", "focal", "focal15_pw", "dice_batch", "focal_tversky_img", "dicebce"])
def test_soft_labels_gradient_of_the_terms(config):
    """Uniform soft labels: the loss to 1e-6, the gradient to RTOL times the sum of the MAGNITUDES of the terms the closed form adds,
    |g| { scale a_t q^gf [ gf |1 - 2y| (p p'/q) ce + pos_weight y sigmoid(-x) + (1 - y) sigmoid(x) ] + (|c1| y + |c0|) p' } in fp64 --
    the gradient itself crosses zero inside the input range (module docstring)."""
    name = "3x1x37x53"
    _, p, g = CONFIGS[config]
    ref_loss, _, _, _, a, b = _reference(name, config, "uniform")
    x, y = (t.double() for t in _inputs(name, "uniform"))
    mag = _magnitudes(x, y, p, g)
    assert bool((mag * (1 + 1e-9) >= (a + b).abs()).all())
    if p["wo"] != 0:                                                  # the closed form of the issue against autograd, in fp64
        c1, c0 = _coefficients(x, y, p)
        assert float(((c1 * y + c0) * _sig(x) * _sig(-x) * g - b).abs().max()) <= 1e-12 * float(mag.max())
    loss, grad, _ = _run(name, config, soft="uniform")
    worst = float(((grad.double().cpu() - (a + b)).abs() / (RTOL * mag + 1e-30)).max())
    rel = abs(float(loss) - ref_loss) / abs(ref_loss)
    print(f"seg loss uniform soft labels {config}: loss rel {rel:.2e}; gradient error / allowance {worst:.3f}")
    assert rel <= 1e-6 and worst <= 1.0


def test_two_runs_are_bit_identical():
    for config in ("focal15_pw", "tversky_img", "dicebce"):
        l1, g1, _ = _run("3x1x37x53", config)
        l2, g2, _ = _run("3x1x37x53", config)
        assert torch.equal(l1, l2) and torch.equal(g1, g2), config


def test_a_misaligned_view_is_bit_identical():
    """The same logits one element into a larger buffer: element accesses where the aligned tensor takes 16-byte ones."""
    name = "2x1x16x24"
    x, _ = _inputs(name)
    buf = torch.empty(x.numel() + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    for config in ("focal", "focal_tversky_img", "dicebce"):
        la, ga, _ = _run(name, config)
        lm, gm, _ = _run(name, config, x_dev=view)
        assert torch.equal(la, lm) and torch.equal(ga, gm), config


def test_default_bce_is_the_bce_of_before_and_a_dropped_term_is_not_evaluated():
    import hyperpri_amd as H
    from hyperpri_amd.trainer import _BCEFn
    x, y = _inputs("3x1x37x53")
    yd = y.to(DEV)

    def run(fn):
        xg = x.to(DEV).requires_grad_(True)
        loss = fn(xg, yd)
        (loss * 3.0).backward()
        return loss.detach(), xg.grad
    l0, g0 = run(_BCEFn.apply)
    l1, g1 = run(H.BCEWithLogitsLoss())
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    # the general family at its BCE point agrees with that kernel to rounding (another summation order)
    l2, g2 = run(H.SegLoss())
    assert abs(float(l2) - float(l0)) <= 1e-6 * float(l0)
    np.testing.assert_allclose(g2.cpu().numpy(), g0.cpu().numpy(), rtol=2e-6, atol=1e-12)
    # overlap weight 0: the bits of the stand-alone pointwise loss; pointwise weight 0: the bits of the stand-alone Dice
    lw, gw = run(H.BCEWithLogitsLoss(pos_weight=3.0))
    ld, gd = run(H.DiceBCELoss(1.0, 0.0, pos_weight=3.0))
    assert torch.equal(lw, ld) and torch.equal(gw, gd)
    lo, go = run(H.DiceLoss(1.0))
    lz, gz = run(H.SegLoss(bce_weight=0.0, overlap_weight=1.0, smooth=0.5, pos_weight=7.0, focal_gamma=2.0))
    assert torch.equal(lo, lz) and torch.equal(go, gz)


def test_shapes_dtypes_and_errors():
    import hyperpri_amd as H
    x, y = _inputs("2x1x16x24")
    xd, yd = x.to(DEV), y.to(DEV)
    crit = H.DiceBCELoss(pos_weight=3.0)
    base = crit(xd, yd)
    for form in (yd.to(torch.uint8), yd.to(torch.int64), yd.double(), yd.bool()):
        assert torch.equal(crit(xd, form), base), form.dtype
    assert torch.equal(crit(xd.view(2, -1), yd.view(2, -1)), base)              # any (N, ...) shape
    with pytest.raises(ValueError, match="must be the same as input size"):
        crit(xd, yd[:, 0])
    with pytest.raises(ValueError, match="must be the same as input size"):
        H.BCEWithLogitsLoss(pos_weight=2.0)(xd, yd[:, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(x, y)
    # an empty foreground without smoothing: D > 0 through P, T = 0; and the all-empty group of the edge rule is finite
    zero = torch.zeros_like(yd)
    xg = xd.clone().requires_grad_(True)
    loss = H.TverskyLoss(0.3, 0.7, 0.0, per_image=True)(xg, zero)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(1.0, rel=1e-6) and bool(torch.isfinite(xg.grad).all())
    xg = torch.full_like(xd, -200.0).requires_grad_(True)                        # every p underflows: I = P = Y = 0, s = 0 -> D == 0
    loss = H.DiceLoss(0.0)(xg, zero)
    loss.backward()
    assert float(loss.detach()) == 0.0 and bool((xg.grad == 0).all())


# ---------------------------------------------------------------------------------------------------
# one training step: UNet(3, 1) under SegmentationModel(net, DiceBCELoss(...))
# ---------------------------------------------------------------------------------------------------
STEP_P = _P(pw=3.0, wo=1.0, s=0.5, per_image=True)


def _oracle_step(sd, x, m, dtype):
    """O.unet_forward in ``dtype``, back-propagated from the fp64 dloss/dlogits of the family: (logits, loss, {name: grad})."""
    leaves, work = OrderedDict(), OrderedDict()
    for k, v in sd.items():
        if O.is_param(k):
            leaves[k] = work[k] = v.detach().to(dtype).clone().requires_grad_(True)
        else:
            work[k] = v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()
    logits = O.unet_forward(work, x.to(dtype))
    l64 = logits.detach().double().requires_grad_(True)
    point, over, _ = _family(l64, m.double(), STEP_P)
    (point + over).backward()
    logits.backward(l64.grad.to(dtype))
    return logits.detach(), float(point + over), OrderedDict((k, p.grad) for k, p in leaves.items())


@functools.lru_cache(maxsize=None)
def _e2e():
    import hyperpri_amd as H
    sd = O.synth_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in H.UNet(3, 1, bilinear=False).state_dict().items()))
    x = _u(1234, (2, 3, 36, 50))
    m = (_u(4321, (2, 1, 36, 50)) > 0.9).float()
    return sd, x, m, _oracle_step(sd, x, m, torch.float32), _oracle_step(sd, x, m, torch.float64)


def test_unet3_one_step_under_dice_bce_matches_the_cpu_oracle(monkeypatch):
    """UNet(3, 1) at (2, 3, 36, 50) in fp32, one training_step of SegmentationModel under DiceBCELoss(pos_weight 3, Dice per image)
    against the fp32 CPU oracle fed with the fp64 dlogits, with the tolerances of
    test_gpu_multiclass.py::test_unet3_three_classes_one_step_matches_the_cpu_oracle: logits 1e-3, loss 1e-5, gradients 2e-3 in
    relative L2 of the difference; convolution biases in front of a train-mode BatchNorm (true gradient 0) are skipped.  The
    weighted criterion must not be replaced by the head's unweighted fused loss."""
    import hyperpri_amd as H
    from hyperpri_amd import trainer as T
    sd, x, m, (ref_logits, ref_loss, ref_grads), (_, _, grads64) = _e2e()
    taken = []
    real = T.forward_loss
    monkeypatch.setattr(T, "forward_loss", lambda *a, **k: (taken.append(1), real(*a, **k))[1])
    net = H.UNet(3, 1, bilinear=False)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    model = H.SegmentationModel(net, H.DiceBCELoss(1.0, 1.0, pos_weight=3.0, smooth=1.0, per_image=True))
    batch = {"image": x.to(DEV), "mask": m.to(DEV)}
    logits, loss = model._step("tr", batch, model.threshold)        # (training_step returns the loss alone)
    loss.backward()
    assert not taken and type(loss.grad_fn).__name__.startswith("_SegLossFn")
    err = float((logits.detach().cpu() - ref_logits).abs().max())
    print(f"unet3 under DiceBCE: max|dlogit| {err:.2e}, loss {float(loss.detach())!r} (oracle {ref_loss!r})")
    assert err < 1e-3
    assert abs(float(loss.detach()) - ref_loss) < 1e-5
    grads = dict(net.named_parameters())
    checked = 0
    for k, ref in ref_grads.items():
        g64 = grads64[k]
        if float(g64.norm()) < 1e-12:                                # mathematically zero: a bias in front of a BatchNorm
            assert k.endswith(".bias")
            continue
        got = grads[k].grad.detach().cpu().double()
        rel = float((got - ref.double()).norm() / ref.double().norm())
        spread = float((ref.double() - g64).norm() / g64.norm())
        print(f"  {k}: relative L2 {rel:.2e} (oracle fp32-fp64 spread {spread:.2e})")
        assert rel <= 2e-3, (k, rel)
        checked += 1
    assert checked >= 55
    assert model.epoch_metrics("tr")["tr_loss"] == pytest.approx(float(loss.detach()), rel=1e-7)
    # the default criterion still takes the fused head
    taken.clear()
    H.SegmentationModel(net).training_step(batch)
    assert taken
