"""precision "torch" (the mode follows torch.autocast / torch.set_float32_matmul_precision, resolved once per forward call) and the
f16 mode's loss scale picked on the device from the incoming gradient.  Gates: a "torch" module is bit-identical to its explicitly set
twin for every row of the resolution table; f16 survives incoming gradients 2^16 and 2^17 times a mean loss's (GradScaler, a
sum-reduced loss) with finite gradients in the f16 band around fp32; the mean loss keeps today's bits; f16 gradient accumulation
under the GradSync sink adds each micro-batch's unscaled gradient once.  Needs a real MI355X: ``-m gpu``."""
import contextlib
import os
import socket
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import record_margin
from oracle import hyperpri_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u(seed, shape):
    return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())


@contextlib.contextmanager
def _matmul(level):
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(level)
    try:
        yield
    finally:
        torch.set_float32_matmul_precision(old)


# ambient state -> the explicit mode it must resolve to (ISSUE table; device type "cuda")
STATES = {
    "autocast_f16": ("f16", lambda: torch.autocast("cuda", torch.float16)),
    "autocast_bf16": ("bf16", lambda: torch.autocast("cuda", torch.bfloat16)),
    "highest": ("fp32", lambda: _matmul("highest")),
    "high": ("bf16x3", lambda: _matmul("high")),
    "medium": ("bf16", lambda: _matmul("medium")),
}

# tiny nets and seeds of tests/test_gpu_nets.py
NETS = {
    "unet3": (lambda H: H.UNet(3, 1, bilinear=False), 1234, (2, 3, 36, 50), 4321, 0.9),
    "cubenet64": (lambda H: H.CubeNET(6, 1, first_depth=64, bilinear=False), 1235, (2, 1, 6, 36, 50), 4321, 0.9),
    "spectral_f50": (lambda H: H.SpectralUNET(22, 1, 50), 1242, (2, 22, 9, 14), 4324, 0.7),
}


def _twin(name, prec, train=True):
    import hyperpri_amd as H
    mk = NETS[name][0]
    net = mk(H)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
    net.load_state_dict(O.synth_state_dict(shapes))
    net = H.set_precision(net.to(DEV), prec)
    return net.train() if train else net.eval()


def _inputs(name):
    _, xs, xshape, ms, thr = NETS[name]
    x = _u(xs, xshape).to(DEV)
    m = (_u(ms, (xshape[0], 1) + tuple(xshape[-2:])) > thr).float().to(DEV)
    return x, m


def _train_step(net, x, m, state=None, bwd_state=None):
    """Forward (and the loss) under ``state``, backward under ``bwd_state`` (default: outside any)."""
    for p in net.parameters():
        p.grad = None
    with (state() if state else contextlib.nullcontext()):
        logits = net(x)
        loss = torch.nn.BCEWithLogitsLoss()(logits, m)
    with (bwd_state() if bwd_state else contextlib.nullcontext()):
        loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach(), [p.grad.detach().clone() for p in net.parameters()]


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a, b), (what, float((a.double() - b.double()).abs().max()))


@pytest.mark.parametrize("state", list(STATES))
@pytest.mark.parametrize("name", list(NETS))
def test_torch_mode_equals_its_explicit_twin_in_training(name, state):
    mode, ctx = STATES[state]
    x, m = _inputs(name)
    a, b = _twin(name, "torch"), _twin(name, mode)
    la, La, ga = _train_step(a, x, m, ctx)
    lb, Lb, gb = _train_step(b, x, m, ctx)
    assert la.dtype == torch.float32
    _same(la, lb, "logits")
    _same(La, Lb, "loss")
    for (k, _), g1, g2 in zip(a.named_parameters(), ga, gb):
        assert g1.dtype == torch.float32
        _same(g1, g2, k)
    for (k, b1), b2 in zip(a.named_buffers(), b.buffers()):
        _same(b1, b2, k)


@pytest.mark.parametrize("state", list(STATES))
@pytest.mark.parametrize("name", list(NETS))
def test_torch_mode_equals_its_explicit_twin_in_inference(name, state):
    mode, ctx = STATES[state]
    x, _ = _inputs(name)
    a, b = _twin(name, "torch", train=False), _twin(name, mode, train=False)
    outs = []
    for net in (a, b):
        with torch.inference_mode(), ctx():
            outs.append(net(x).clone())
    torch.cuda.synchronize()
    assert outs[0].dtype == torch.float32
    _same(outs[0], outs[1], "logits")


def test_mode_is_fixed_per_call():
    """The ambient state at backward time does not matter, and one module run under four states in a row matches a fresh explicit
    twin every time (no packed weight or library choice leaks from one call's mode into the next)."""
    x, m = _inputs("cubenet64")
    a = _twin("cubenet64", "torch")
    _, _, g_ref = _train_step(_twin("cubenet64", "f16"), x, m, STATES["autocast_f16"][1])
    _, _, g = _train_step(a, x, m, STATES["autocast_f16"][1], bwd_state=STATES["high"][1])
    for (k, _), g1, g2 in zip(a.named_parameters(), g, g_ref):
        _same(g1, g2, k)
    _, _, g = _train_step(a, x, m, STATES["highest"][1], bwd_state=STATES["autocast_bf16"][1])
    _, _, g_ref = _train_step(_twin("cubenet64", "fp32"), x, m, STATES["highest"][1])
    for (k, _), g1, g2 in zip(a.named_parameters(), g, g_ref):
        _same(g1, g2, k)
    for state in ("autocast_bf16", "high", "autocast_f16", "medium"):
        mode, ctx = STATES[state]
        la, _, ga = _train_step(a, x, m, ctx)
        lb, _, gb = _train_step(_twin("cubenet64", mode), x, m, ctx)
        _same(la, lb, f"{state}: logits")
        for (k, _), g1, g2 in zip(a.named_parameters(), ga, gb):
            _same(g1, g2, f"{state}: {k}")


# ---- f16 under large incoming gradients ----------------------------------------------------------------------------------------------
BIG = ((2, 1, 6, 256, 256), 1235, 4321, 0.9)        # 2 x 256 x 256 = 2^17 logits: the static scale is 2^17


def _big():
    shape, xs, ms, thr = BIG
    x = _u(xs, shape).to(DEV)
    m = (_u(ms, (shape[0], 1) + shape[-2:]) > thr).float().to(DEV)
    return x, m


def _rel_err(g16, g32):
    """max over the weight tensors (dim > 1) of |g16 - g32|_2 / |g32|_2 (biases ahead of a training-mode BatchNorm have a true
    gradient of 0: both sides are rounding noise there)."""
    worst = 0.0
    for a, b in zip(g16, g32):
        if b.dim() > 1:
            worst = max(worst, float((a.double() - b.double()).norm() / b.double().norm()))
    return worst


# f16 against fp32 on the 2^17-logit CubeNET, worst weight tensor: measured 0.19 under the sum loss, 65536 x the mean loss and
# GradScaler alike (the picked scales are powers of two: the same relative error); measured + 50 %
F16_REL_TOL = 0.29


def _grads(prec, loss_fn):
    x, m = _big()
    net = _twin("cubenet64", prec)
    for p in net.parameters():
        p.grad = None
    loss_fn(net(x), m).backward()
    torch.cuda.synchronize()
    return [p.grad.detach().clone() for p in net.parameters()]


LOSSES = {
    "sum": lambda y, m: torch.nn.BCEWithLogitsLoss(reduction="sum")(y, m),
    "mean_x65536": lambda y, m: 65536 * torch.nn.BCEWithLogitsLoss()(y, m),
}


@pytest.mark.parametrize("loss", list(LOSSES))
def test_f16_survives_large_incoming_gradients(loss):
    g16 = _grads("f16", LOSSES[loss])
    for i, g in enumerate(g16):
        assert torch.isfinite(g).all(), (loss, i)
    g32 = _grads("fp32", LOSSES[loss])
    err = _rel_err(g16, g32)
    record_margin(f"amp/f16_vs_fp32/{loss}", err, F16_REL_TOL)
    assert err < F16_REL_TOL, (loss, err)


def test_f16_mean_loss_is_bit_identical_under_both_scale_rules():
    from hyperpri_amd import engine as E
    x, m = _inputs("cubenet64")
    old = E.F16_LOSS_SCALE
    try:
        E.F16_LOSS_SCALE = "static"
        _, _, g_static = _train_step(_twin("cubenet64", "f16"), x, m)
        E.F16_LOSS_SCALE = "adaptive"
        _, _, g_adapt = _train_step(_twin("cubenet64", "f16"), x, m)
    finally:
        E.F16_LOSS_SCALE = old
    for i, (a, b) in enumerate(zip(g_static, g_adapt)):
        _same(a, b, str(i))


def _amp_step(prec, opt_kind, autocast):
    """One GradScaler step of the 2^17-logit CubeNET; returns (scale after update, unscaled gradients, parameters moved?)."""
    import hyperpri_amd as H
    x, m = _big()
    net = _twin("cubenet64", prec)
    before = [p.detach().clone() for p in net.parameters()]
    opt = H.FusedAdam(net.parameters(), lr=1e-3) if opt_kind == "fused" else torch.optim.Adam(net.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda")
    assert scaler.get_scale() == 65536.0
    with (torch.autocast("cuda", torch.float16) if autocast else contextlib.nullcontext()):
        loss = torch.nn.BCEWithLogitsLoss()(net(x), m)
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    grads = [p.grad.detach().clone() for p in net.parameters()]
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    moved = all(not torch.equal(p.detach(), q) for p, q in zip(net.parameters(), before) if p.dim() > 1)
    return scaler.get_scale(), grads, moved


@pytest.mark.parametrize("opt_kind", ["fused", "torch"])
def test_amp_end_to_end_with_grad_scaler(opt_kind):
    scale, grads, moved = _amp_step("torch", opt_kind, autocast=True)
    assert scale == 65536.0, "GradScaler skipped the first step (non-finite gradients)"
    assert moved
    for i, g in enumerate(grads):
        assert torch.isfinite(g).all(), i
    g32 = _grads("fp32", lambda y, t: torch.nn.BCEWithLogitsLoss()(y, t))
    err = _rel_err(grads, g32)
    record_margin(f"amp/grad_scaler/{opt_kind}", err, F16_REL_TOL)
    assert err < F16_REL_TOL, err
    # the explicit f16 twin under the same GradScaler takes the same step (it skipped it while the scale was fixed on the host)
    scale_e, grads_e, moved_e = _amp_step("f16", opt_kind, autocast=False)
    assert scale_e == 65536.0 and moved_e
    for g1, g2 in zip(grads, grads_e):
        _same(g1, g2, "explicit twin")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.parametrize("prec", ["fp32", "bf16", "f16"])
def test_accumulation_under_the_sink_adds_each_micro_batch_once(tmp_path, prec):
    out = str(tmp_path / "rank.npz")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4", GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_amp_sink_rank.py"), str(_free_port()), out, prec], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-3000:]
    z = np.load(out)
    assert int(z["buckets"]) > 1
    names = [k[len("acc/"):] for k in z.files if k.startswith("acc/")]
    worst = 0.0
    for k in names:
        want = torch.from_numpy(z["step0/" + k]) + torch.from_numpy(z["step1/" + k])     # fp32 sum of the single-step gradients
        got = torch.from_numpy(z["acc/" + k])
        if prec == "f16":
            _same(got, want, k)
        else:
            # the accumulating kernels of fp32 / bf16 may add partial sums in another order: fp32 rounding of the sum
            d = float((got.double() - want.double()).abs().max())
            ref = float(want.double().abs().max())
            worst = max(worst, d / (ref + 1e-30))
            assert d <= 1e-5 * ref + 1e-7, (k, d, ref)
    record_margin(f"amp/sink_accumulation/{prec}", worst, 1e-5)
