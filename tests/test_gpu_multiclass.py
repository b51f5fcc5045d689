"""The multi-class tail on the device (csrc/multiclass.hip, hpri_segmap_classes; trainer.CrossEntropyLoss / SegConfusion /
SegmentationModel(task="multiclass"), evaluate.evaluate_multiclass / color_classmaps) against torch on the CPU.

Tolerances.  Loss: 1e-6 relative against nn.CrossEntropyLoss in fp64 over the same fp32 inputs (the gate of
test_bce_with_logits_matches_torch_cpu).  Gradients: rtol 4e-6, atol 1e-12 per element against fp64 -- for |x| <= 8 the exponent
x_k - lse is rounded at 16 * 2^-24 ~ 9.5e-7, plus about two ulp of expf, K/2 ulp of the sum and two divisions, the total
doubled.  Class maps, confusion counts and ignored / invalid gradients are integers or exact zeros: exact.  Pictures: within one
level per channel, the rule of test_gpu_evaluate.py.  Needs a real MI355X."""
import functools
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hyperpri_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IGNORE = 255


def _u(seed, shape):
    return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())


def _targets(seed, shape, K):
    """(N, h, w) int64 class indices from O._u."""
    return (_u(seed, shape) * K).long().clamp(max=K - 1)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """Logits in [-8, 8) with a few planted confident pixels (+-40 on the target class and on another one, and a moderate
    +14 on the target), int64 targets, and a mask of about 10 % of the pixels to ignore."""
    N, K, h, w = shape
    x = _u(201, shape) * 16 - 8
    t = _targets(202, (N, h, w), K)
    flat = x.permute(0, 2, 3, 1).reshape(-1, K)                     # a copy: pixel-major rows
    tf = t.reshape(-1)
    npix = tf.numel()
    plant = [(3, 40.0, -40.0), (7, -40.0, 40.0), (npix - 1, 40.0, 40.0), (npix // 2, -40.0, -40.0), (11, 14.0, None)]
    for p, vt, vo in plant:
        p = p % npix
        cls = int(tf[p])
        flat[p, cls] = vt
        if vo is not None:
            flat[p, (cls + 1) % K] = vo
    x = flat.reshape(N, h, w, K).permute(0, 3, 1, 2).contiguous()
    ignore = _u(203, (N, h, w)) < 0.1
    ignore.reshape(-1)[[1, npix - 2]] = True                        # (the 15-pixel case draws none)
    ignore.reshape(-1)[[3, 11]] = False                             # the planted pixels keep counting
    return x, t, ignore


CONFIGS = {
    # name: (weighted, ignore, reduction, target dtype, upstream gradient)
    "plain": (False, False, "mean", torch.int64, 1.0),
    "weighted": (True, False, "mean", torch.float32, 2.5),
    "ignore": (True, True, "mean", torch.uint8, 1.0),
    "sum": (False, True, "sum", torch.int32, 0.37),
}


def _weight(K):
    return 0.25 + 1.5 * _u(204, (K,))


@functools.lru_cache(maxsize=None)
def _reference(shape, config):
    """(loss, dlogits) of nn.CrossEntropyLoss on the CPU in fp64 over the same fp32 inputs; computed once per case."""
    weighted, ignore, reduction, _, g = CONFIGS[config]
    x, t, ign = _inputs(shape)
    t = torch.where(ign, torch.full_like(t, IGNORE), t) if ignore else t
    xd = x.double().requires_grad_(True)
    crit = torch.nn.CrossEntropyLoss(weight=_weight(shape[1]).double() if weighted else None, ignore_index=IGNORE if ignore else -100,
                                     reduction=reduction)
    loss = crit(xd, t)
    (loss * g).backward()
    return float(loss.detach()), xd.grad


def _run(shape, config, x_dev=None):
    """The device loss, dlogits and target for one case."""
    import hyperpri_amd as H
    weighted, ignore, reduction, tdtype, g = CONFIGS[config]
    x, t, ign = _inputs(shape)
    t = torch.where(ign, torch.full_like(t, IGNORE), t) if ignore else t
    xg = (x.to(DEV) if x_dev is None else x_dev).detach().requires_grad_(True)
    crit = H.CrossEntropyLoss(weight=_weight(shape[1]) if weighted else None, ignore_index=IGNORE if ignore else -100,
                              reduction=reduction).to(DEV)
    tg = t.to(tdtype).to(DEV)
    loss = crit(xg, tg)
    (loss * g).backward()
    again = crit(xg.detach(), tg)
    return loss.detach(), xg.grad, again, t


SHAPES = [(1, 3, 3, 5), (2, 7, 36, 50), (2, 19, 36, 50), (2, 4, 608, 968)]


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_cross_entropy_matches_torch_cpu_fp64(shape, config):
    """(1,3,3,5): HW = 15, the element path and a short last quad; (2,7,36,50): 16-byte path; (2,19,36,50): runtime K;
    (2,4,608,968): more quads than one grid-stride sweep (1024 blocks of 256 lanes)."""
    ref_loss, ref_grad = _reference(shape, config)
    loss, grad, again, t = _run(shape, config)
    got = float(loss)
    rel = abs(got - ref_loss) / abs(ref_loss)
    err = (grad.double().cpu() - ref_grad).abs()
    worst = float((err / (1e-12 + 4e-6 * ref_grad.abs())).max())
    print(f"cross-entropy {shape} {config}: loss {got!r} (fp64 {ref_loss!r}, rel {rel:.2e}); gradient error / allowance {worst:.3f}")
    assert rel <= 1e-6
    assert worst <= 1.0
    assert torch.equal(again, loss)                                  # a second forward: bit-identical
    if CONFIGS[config][1]:
        ignored = (t == IGNORE).unsqueeze(1).expand_as(grad)
        assert bool(ignored.any()) and bool((grad.cpu()[ignored] == 0).all())
        assert not bool(torch.signbit(grad.cpu()[ignored]).any())    # +0, not -0
    # the planted confident pixel: its target-class gradient is a tiny non-zero number, not the 0 of p_t - 1
    N, K, h, w = shape
    p = 3
    if K > 2 or CONFIGS[config][2] == "sum":
        n, y, xx = 0, p // w, p % w
        cls = int(t[n, y, xx])
        assert float(grad[n, cls, y, xx]) < 0.0


def test_cross_entropy_from_a_misaligned_view_is_bit_identical():
    """The same logits as a contiguous view one element into a larger buffer: every plane starts 4 bytes off a 16-byte boundary,
    so the element path runs where the aligned tensor takes 16-byte accesses."""
    shape = (2, 7, 36, 50)
    x, _, _ = _inputs(shape)
    buf = torch.empty(x.numel() + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + x.numel()].view(shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    for config in ("weighted", "ignore"):
        loss_a, grad_a, _, _ = _run(shape, config)
        loss_m, grad_m, _, _ = _run(shape, config, x_dev=view)
        assert torch.equal(loss_a, loss_m) and torch.equal(grad_a, grad_m)


def test_cross_entropy_target_forms_and_errors():
    import hyperpri_amd as H
    shape = (2, 7, 36, 50)
    N, K, h, w = shape
    x, t, _ = _inputs(shape)
    xd = x.to(DEV)
    crit = H.CrossEntropyLoss()
    base = crit(xd, t.to(DEV))
    for form in (t.to(torch.uint8), t.float(), t.to(torch.int32), t.to(torch.int16), t.double(), t.unsqueeze(1), t.float().unsqueeze(1)):
        assert torch.equal(crit(xd, form.to(DEV)), base), (form.dtype, tuple(form.shape))
    with pytest.raises(ValueError, match="target of shape"):
        crit(xd, t[:, :-1].to(DEV))
    with pytest.raises(ValueError, match="classes"):
        crit(torch.zeros(1, 1, 4, 4, device=DEV), torch.zeros(1, 4, 4, device=DEV))
    with pytest.raises(ValueError, match="classes"):
        crit(torch.zeros(1, 65, 4, 4, device=DEV), torch.zeros(1, 4, 4, device=DEV))
    with pytest.raises(ValueError, match="weight"):
        H.CrossEntropyLoss(weight=torch.ones(K + 1)).to(DEV)(xd, t.to(DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(xd, t)


@pytest.mark.parametrize("tdtype,bad", [(torch.int64, 7), (torch.int64, -1), (torch.uint8, 200), (torch.float32, 7.0),
                                        (torch.float32, float("nan")), (torch.float32, 1e30), (torch.int64, 1 << 40)])
def test_an_invalid_target_poisons_the_loss_without_a_fault(tdtype, bad):
    import hyperpri_amd as H
    shape = (2, 7, 36, 50)
    x, t, _ = _inputs(shape)
    tg = t.to(tdtype).clone()                                        # (the cached inputs stay as they are)
    tg[1, 17, 23] = bad
    xg = x.to(DEV).requires_grad_(True)
    loss = H.CrossEntropyLoss(weight=_weight(7)).to(DEV)(xg, tg.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss))
    g = xg.grad.cpu()
    assert bool((g[1, :, 17, 23] == 0).all())                        # the invalid pixel: zeros
    rest = torch.ones(shape, dtype=torch.bool)
    rest[1, :, 17, 23] = False
    assert bool(torch.isfinite(g[rest]).all())
    # and the device still works
    assert float(H.CrossEntropyLoss()(x.to(DEV), t.to(DEV))) > 0


def test_an_all_ignored_batch_is_nan_like_torch():
    import hyperpri_amd as H
    x = (_u(211, (2, 5, 6, 10)) * 16 - 8)
    t = torch.full((2, 6, 10), IGNORE, dtype=torch.int64)
    assert bool(torch.isnan(torch.nn.CrossEntropyLoss(ignore_index=IGNORE)(x.double(), t)))
    xg = x.to(DEV).requires_grad_(True)
    loss = H.CrossEntropyLoss(ignore_index=IGNORE)(xg, t.to(DEV))
    loss.backward()
    assert bool(torch.isnan(loss)) and bool((xg.grad == 0).all())
    total = H.CrossEntropyLoss(ignore_index=IGNORE, reduction="sum")(xg.detach(), t.to(DEV))
    assert float(total) == 0.0


# ---------------------------------------------------------------------------------------------------
# argmax + confusion matrix
# ---------------------------------------------------------------------------------------------------
def _confusion_case(shape, seed):
    """Logits with planted ties (between two maxima, and between all classes), NaNs (one, and two in one pixel) and uint8 targets with
    about 10 % of the pixels ignored."""
    N, K, h, w = shape
    x = _u(seed, shape) * 16 - 8
    x[0, 1, 2, 3] = x[0, K - 1, 2, 3] = 9.0                          # two equal maxima: the lower index wins
    x[N - 1, :, h - 1, w - 1] = 1.5                                  # all equal: class 0
    x[0, 2, 5, 7] = float("nan")                                     # a NaN counts as the maximum
    x[N - 1, 1, 0, 1] = x[N - 1, 3, 0, 1] = float("nan")             # the first NaN wins
    x[0, 0, 0, 0] = float("inf")
    x[0, K - 1, 0, 2] = float("inf")
    t = _targets(seed + 1, (N, h, w), K)
    t[_u(seed + 2, (N, h, w)) < 0.1] = IGNORE
    return x, t.to(torch.uint8)


def _histogram(pred, t, K):
    keep = t != IGNORE
    return np.bincount((t[keep].long() * K + pred[keep]).numpy(), minlength=K * K).reshape(K, K)


@pytest.mark.parametrize("shape", [(2, 5, 36, 50), (2, 4, 608, 968)], ids=["2x5x36x50", "2x4x608x968"])
def test_confusion_matrix_and_class_map_equal_torch_argmax(shape):
    import hyperpri_amd as H
    N, K, h, w = shape
    x1, t1 = _confusion_case(shape, 221)
    x2, t2 = _confusion_case(shape, 231)
    p1, p2 = torch.argmax(x1, 1), torch.argmax(x2, 1)
    assert int(p1[0, 2, 3]) == 1 and int(p1[N - 1, h - 1, w - 1]) == 0 and int(p1[0, 5, 7]) == 2 and int(p1[N - 1, 0, 1]) == 1
    want = _histogram(p1, t1, K) + _histogram(p2, t2, K)
    conf = H.SegConfusion(K, ignore_index=IGNORE)
    classes = torch.empty((N, h, w), dtype=torch.uint8, device=DEV)
    conf.update(x1.to(DEV), t1.to(DEV), classes=classes)
    assert torch.equal(classes.cpu().long(), p1)
    assert np.array_equal(np.asarray(conf.matrix()), _histogram(p1, t1, K))
    conf.update(x2.to(DEV), t2.unsqueeze(1).float().to(DEV))          # accumulates; another target form
    got = conf.compute()
    assert np.array_equal(got["confusion"], want) and int(want.sum()) == int((t1 != IGNORE).sum() + (t2 != IGNORE).sum())
    assert got["acc"] == pytest.approx(np.trace(want) / want.sum(), rel=1e-12)
    assert torch.equal(H.argmax_classes(x2.to(DEV)).cpu().long(), p2)
    # the element path (a view 4 bytes off a 16-byte boundary) decides the same
    buf = torch.empty(x1.numel() + 8, dtype=torch.float32, device=DEV)
    view = buf[1:1 + x1.numel()].view(shape)
    view.copy_(x1)
    assert torch.equal(H.argmax_classes(view).cpu().long(), p1)
    conf.reset()
    assert not np.asarray(conf.matrix()).any()


def test_confusion_raises_after_an_invalid_target():
    import hyperpri_amd as H
    shape = (1, 3, 3, 5)                                              # HW = 15: element path, short last quad
    x = _u(241, shape) * 16 - 8
    t = _targets(242, (1, 3, 5), 3)
    conf = H.SegConfusion(3)
    conf.update(x.to(DEV), t.to(DEV))
    assert np.array_equal(conf.compute()["confusion"], _histogram(torch.argmax(x, 1), t, 3))
    t[0, 2, 4] = 3
    conf.update(x.to(DEV), t.to(DEV))
    with pytest.raises(ValueError, match="neither inside"):
        conf.compute()
    with pytest.raises(ValueError, match="built for 3 classes"):
        conf.update(torch.zeros(1, 4, 3, 5, device=DEV), t.to(DEV))


# ---------------------------------------------------------------------------------------------------
# class maps
# ---------------------------------------------------------------------------------------------------
def _restate_classmap(image, cls, palette, alpha, bands, gamma):
    """hpri_segmap_classes' arithmetic in fp32 on the host, with the library's clamp / NaN rule (as test_gpu_evaluate._restate)."""
    v = torch.nan_to_num(image[:, list(bands)].float(), nan=0.0).clamp(0, 1)
    base = (v if gamma == 1 else v ** (1 / gamma)).permute(0, 2, 3, 1)
    table = torch.tensor(palette, dtype=torch.float32)
    c = cls.long()
    c = torch.where(c < len(palette), c, torch.zeros_like(c))
    a = torch.tensor(alpha, dtype=torch.float32)
    out = torch.where((c == 0).unsqueeze(-1), base, a * table[c] + (1 - a) * base)
    return (out * 255 + 0.5).to(torch.uint8)


def test_color_classmaps_contiguous_image():
    import hyperpri_amd as H
    N, C, h, w = 2, 6, 9, 13                                          # w = 13: three quads and a tail; 9 * 13 odd: every alignment
    K, bands = 5, (4, 0, 2)
    img = _u(251, (N, C, h, w)) * 1.2 - 0.1
    img[0, 0, 1, 2] = float("nan")
    cls = (_u(252, (N, h, w)) * K).to(torch.uint8).clamp(max=K - 1)
    cls[1, 8, 12] = 200                                               # beyond the palette: paints as class 0
    cls[0, 0, 0] = K
    pal = H.default_class_palette(K)
    for alpha, gamma in ((0.6, 2.2), (1.0, 1.0), (0.0, 2.2)):
        rgb = H.color_classmaps(img.to(DEV), cls.to(DEV), palette=pal, alpha=alpha, bands=bands, gamma=gamma)
        assert rgb.dtype == torch.uint8 and rgb.is_cuda and tuple(rgb.shape) == (N, h, w, 3)
        want = _restate_classmap(img, cls, pal, alpha, bands, gamma)
        diff = int((rgb.cpu().int() - want.int()).abs().max())
        print(f"class map {(N, C, h, w)} alpha {alpha} gamma {gamma}: max level difference {diff}")
        assert diff <= 1
    # the defaults: bands (125, 49, 0) / gamma 2.2 need more than three bands -- this image takes them only when told
    flat = H.color_classmaps(img[:, :3].contiguous().to(DEV), cls.unsqueeze(1).long().to(DEV), alpha=1.0)
    want = _restate_classmap(img[:, :3], cls, H.default_class_palette(64), 1.0, (0, 1, 2), 1.0)
    assert int((flat.cpu().int() - want.int()).abs().max()) <= 1
    painted = (cls > 0) & (cls < K)
    levels = (torch.tensor(pal) * 255 + 0.5).to(torch.uint8)
    assert torch.equal(flat.cpu()[painted], levels[cls[painted].long()])       # alpha = 1: the bare colours, exactly


def test_color_classmaps_channels_last_cube_view():
    import hyperpri_amd as H
    N, C, cs, h, w = 1, 6, 8, 12, 16
    buf = torch.zeros(N, h, w, cs)
    buf[..., :C] = _u(261, (N, h, w, C))
    dev = buf.to(DEV)
    image = dev[:, :, :, :C].permute(0, 3, 1, 2).unsqueeze(1)         # (1, 1, 6, 12, 16), as the cube cache hands it out
    assert tuple(image.shape) == (1, 1, 6, 12, 16) and image.stride()[2:] == (1, w * cs, cs)
    K, bands = 4, (5, 2, 0)
    cls = (_u(262, (N, h, w)) * K).to(torch.uint8).clamp(max=K - 1)
    rgb = H.color_classmaps(image, cls.to(DEV), palette=H.default_class_palette(K), bands=bands, gamma=2.2)
    want = _restate_classmap(buf[..., :C].permute(0, 3, 1, 2), cls, H.default_class_palette(K), 0.6, bands, 2.2)
    diff = int((rgb.cpu().int() - want.int()).abs().max())
    print(f"class map of a cube view: max level difference {diff}")
    assert diff <= 1
    assert sorted(cls.unique().tolist()) == [0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------------
# end to end: UNet(3, 3) under CrossEntropyLoss
# ---------------------------------------------------------------------------------------------------
def _oracle_step(sd, x, t, dtype):
    """O.train_step with F.cross_entropy in place of the BCE, in ``dtype``: (logits, loss, {name: grad})."""
    leaves, work = OrderedDict(), OrderedDict()
    for k, v in sd.items():
        if O.is_param(k):
            leaves[k] = work[k] = v.detach().to(dtype).clone().requires_grad_(True)
        else:
            work[k] = v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()
    logits = O.unet_forward(work, x.to(dtype))
    loss = F.cross_entropy(logits, t)
    loss.backward()
    return logits.detach(), float(loss.detach()), OrderedDict((k, p.grad) for k, p in leaves.items())


@functools.lru_cache(maxsize=None)
def _e2e():
    import hyperpri_amd as H
    sd = O.synth_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in H.UNet(3, 3, bilinear=False).state_dict().items()))
    x = _u(1234, (2, 3, 36, 50))
    t = _targets(4321, (2, 36, 50), 3)
    return sd, x, t, _oracle_step(sd, x, t, torch.float32), _oracle_step(sd, x, t, torch.float64)


def _net(sd):
    import hyperpri_amd as H
    net = H.UNet(3, 3, bilinear=False)
    net.load_state_dict(sd)
    return net.to(DEV).train()


def test_unet3_three_classes_one_step_matches_the_cpu_oracle():
    """UNet(3, 3) at (2, 3, 36, 50), the geometry of net_unet3_tiny, one step under CrossEntropyLoss against the fp32 CPU oracle
    (O.unet_forward + F.cross_entropy): logits 1e-3, loss 1e-5, gradients 2e-3 in relative L2 of the difference.

    Measured before fixing the gradient gate (CPU, the oracle in fp32 against the oracle in fp64, relative L2 of the difference per
    tensor): 2.8e-3 .. 4.5e-3 for every convolution weight and BatchNorm parameter from ``inc`` to ``up4.conv.double_conv.3``,
    6.8e-4 .. 3.6e-3 for the transposed convolutions' biases, 9.7e-4 for ``up4.conv.double_conv.4.bias``; only
    ``up4.conv.double_conv.4.weight`` (3.6e-7), ``outc.conv.weight`` (4.2e-7) and ``outc.conv.bias`` (4.1e-7) lie under a third of
    2e-3.  By the rule set for this test a tensor whose spread exceeds 2e-3 / 3 may be held to three times its spread (8e-3 ..
    1.35e-2 here).  The device turned out to agree with the fp32 oracle to 2e-7 .. 8e-6 on every tensor (one MI355X), so the
    test keeps the plain 2e-3 for ALL tensors -- never wider than the rule allows -- and prints the spread, recomputed from the two
    oracle runs, beside each figure.  Convolution biases in front of a train-mode BatchNorm have a true gradient of 0 (|g| ~ 1e-17
    in fp64): skipped."""
    import hyperpri_amd as H
    sd, x, t, (ref_logits, ref_loss, ref_grads), (_, _, grads64) = _e2e()
    net = _net(sd)
    logits = net(x.to(DEV))
    loss = H.CrossEntropyLoss()(logits, t.to(DEV))
    loss.backward()
    err = float((logits.detach().cpu() - ref_logits).abs().max())
    print(f"unet3 x 3 classes: max|dlogit| {err:.2e}, loss {float(loss.detach())!r} (oracle {ref_loss!r})")
    assert err < 1e-3
    assert abs(float(loss.detach()) - ref_loss) < 1e-5
    grads = dict(net.named_parameters())
    checked = 0
    for k, ref in ref_grads.items():
        g64 = grads64[k]
        if float(g64.norm()) < 1e-12:                                # mathematically zero: a bias in front of a BatchNorm
            assert k.endswith(".bias")
            continue
        spread = float((ref.double() - g64).norm() / g64.norm())
        gate = 2e-3                                                  # (the rule would allow max(2e-3, 3 * spread))
        got = grads[k].grad.detach().cpu().double()
        rel = float((got - ref.double()).norm() / ref.double().norm())
        print(f"  {k}: relative L2 {rel:.2e} (oracle fp32-fp64 spread {spread:.2e}, gate {gate:.2e})")
        assert rel <= gate, (k, rel, gate)
        checked += 1
    assert checked >= 55

    # the same step through SegmentationModel: the same loss, and the epoch's metrics from the step's confusion matrix
    net2 = _net(sd)
    model = H.SegmentationModel(net2, task="multiclass", num_classes=3)
    loss2 = model.training_step({"image": x.to(DEV), "mask": t.unsqueeze(1).float().to(DEV)})
    assert torch.equal(loss2.detach(), loss.detach())
    pred = torch.argmax(logits.detach().cpu(), 1)
    want = H.multiclass_metrics_from_confusion(np.bincount((t * 3 + pred).reshape(-1).numpy(), minlength=9).reshape(3, 3))
    got = model.epoch_metrics("tr")
    assert got["tr_loss"] == pytest.approx(float(loss.detach()), rel=1e-7)
    for k in ("acc", "mean_iou", "mean_dice"):
        assert got[f"tr_{k}"] == pytest.approx(want[k], rel=1e-12) and got[f"tr_{k}_pooled"] == pytest.approx(want[k], rel=1e-12)
    np.testing.assert_allclose(got["tr_iou_per_class_pooled"], want["iou_per_class"], rtol=1e-12)
    assert model.epoch_metrics("tr") == {}                           # reset


def test_evaluate_multiclass_over_ragged_batches(tmp_path):
    import hyperpri_amd as H
    sd, x, t, _, _ = _e2e()
    net = _net(sd)
    xs = torch.cat([x, _u(1299, (1, 3, 36, 50))])                     # three images: a batch of 2 and one of 1
    ts = torch.cat([t, _targets(4399, (1, 36, 50), 3)])
    ts[0, :4, :9] = IGNORE
    names = ["plant_a", "plant_b", "plant_c"]
    weight = _weight(3)
    batches = [{"image": xs[a:b].to(DEV), "mask": ts[a:b].to(torch.uint8).to(DEV), "index": names[a:b]} for a, b in ((0, 2), (2, 3))]
    net.eval()
    with torch.no_grad():
        logits = torch.cat([net(b["image"]) for b in batches]).cpu()
    net.train()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    out = H.evaluate_multiclass(net, batches, 3, ignore_index=IGNORE, class_weight=weight, segmap_dir=str(tmp_path / "maps"))
    assert net.training and all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    pred = torch.argmax(logits, 1)
    assert np.array_equal(out["confusion"], _histogram(pred, ts, 3))
    want = H.multiclass_metrics_from_confusion(_histogram(pred, ts, 3))
    assert out["mean_iou"] == want["mean_iou"] and out["mean_dice"] == want["mean_dice"] and out["acc"] == want["acc"]
    ref = float(F.cross_entropy(logits.double(), ts, weight=weight.double(), ignore_index=IGNORE))
    print(f"evaluate_multiclass: ce_loss {out['ce_loss']!r} (fp64 {ref!r})")
    assert abs(out["ce_loss"] - ref) <= 1e-6 * abs(ref)
    assert out["names"] == names
    try:
        from PIL import Image
        ext, read = ".png", lambda p: np.asarray(Image.open(p).convert("RGB"))
    except ImportError:
        ext, read = ".npy", np.load
    assert sorted(os.listdir(tmp_path / "maps")) == [f"{nm}_seg{ext}" for nm in names]
    assert out["paths"] == [str(tmp_path / "maps" / f"{nm}_seg{ext}") for nm in names]
    direct = H.color_classmaps(xs.to(DEV), pred.to(torch.uint8).to(DEV), palette=H.default_class_palette(3)).cpu().numpy()
    for i, path in enumerate(out["paths"]):
        assert np.array_equal(read(path), direct[i])
    with pytest.raises(ValueError, match="neither inside"):           # without the ignore_index, 255 is no class
        H.evaluate_multiclass(net, batches, 3)
