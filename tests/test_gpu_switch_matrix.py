"""Pairwise matrix of the documented switches (twelve environment switches) on tiny
networks: every PAIR of the switches that change which kernels run is set to its non-default value together, in every precision
mode the pair applies to, and one training step must stay finite and inside the mode's band around the all-defaults step.  Free
allocator blocks are poisoned with NaN first, so a kernel that reads a tensor another switch stopped writing shows up as a
non-finite value (the round-2 advisor's silent-wrong-dW finding was exactly such a pair).  Needs a real MI355X: ``-m gpu``."""
import itertools
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import record_margin
from oracle import hyperpri_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FUSION_ATTRS = ("PLANES_ONLY_GRAD", "PLANES_ONLY_ACT", "PLANES_LAZY", "PLANES_CONCAT", "PLANES_CONVT", "YR_BF16", "FUSE_BN_REDUCE",
                "COLSUM_FROM_STATS", "CONVT_PLANES", "GRAD_BF16_INNER", "PLANES_CAT1")
# switch -> (module, attributes, non-default value, precision modes it matters in)
SWITCHES = {
    "HPRI_WINOGRAD": ("engine", ("WINOGRAD", "WINO_WGRAD"), False, ("fp32",)),
    "HPRI_SIDE_STREAM": ("engine", ("SIDE_STREAM",), False, ("fp32", "bf16", "bf16x3")),
    "HPRI_PLANE_CONV": ("engine", ("PLANE_CONV",), False, ("bf16",)),
    "HPRI_PLANE_WGRAD": ("engine", ("PLANE_WGRAD",), False, ("bf16",)),
    "HPRI_PLANE_GEMM": ("engine", ("PLANE_GEMM",), False, ("bf16",)),
    "HPRI_FUSIONS": ("engine", ("FUSIONS",) + FUSION_ATTRS, False, ("fp32", "bf16")),
    "HPRI_PACK_CACHE": ("engine", ("PACK_CACHE",), False, ("fp32", "bf16")),
    "HPRI_DISPATCHER": ("autograd", ("USE_DISPATCHER",), False, ("fp32", "bf16")),
}
# relative L2 of a gradient tensor against the all-defaults run of the same precision mode: fp32 paths differ by summation order
# only; two correct bf16 paths on these tiny, ill-conditioned nets differ by up to ~0.3 (tests/test_gpu_round2.py)
BAND = {"fp32": 2e-3, "bf16": 0.7, "bf16x3": 2e-3}


def _u(seed, shape):
    return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())


def _nets():
    import hyperpri_amd as H
    out = {}
    for kind in ("cube64", "spectral"):
        if kind == "cube64":
            net, x, m = H.CubeNET(6, 1, first_depth=64, bilinear=False), _u(1235, (2, 1, 6, 36, 50)), (_u(4321, (2, 1, 36, 50)) > 0.9).float()
        else:
            net, x, m = H.SpectralUNET(10, 1, 36), _u(1237, (2, 10, 12, 20)), (_u(4322, (2, 1, 12, 20)) > 0.9).float()
        shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
        net.load_state_dict(O.synth_state_dict(shapes))
        out[kind] = (net.to(DEV).train(), x.to(DEV), m.to(DEV))
    return out


def _step(net, x, m, sd):
    net.load_state_dict(sd)
    junk = [torch.full((16 << 20,), float("nan"), device=DEV) for _ in range(4)]      # NaN into the allocator's free pool
    del junk
    for p in net.parameters():
        p.grad = None
    logits = net(x)
    torch.nn.BCEWithLogitsLoss()(logits, m).backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), [p.grad.detach().clone() for p in net.parameters()]


class _Set:
    def __init__(self, names):
        import hyperpri_amd.autograd as A
        import hyperpri_amd.engine as E
        self.mods = {"engine": E, "autograd": A}
        self.names = names

    def __enter__(self):
        self.saved = []
        for n in self.names:
            mod, attrs, val, _ = SWITCHES[n]
            for a in attrs:
                self.saved.append((self.mods[mod], a, getattr(self.mods[mod], a)))
                setattr(self.mods[mod], a, val)

    def __exit__(self, *exc):
        for mod, a, v in reversed(self.saved):
            setattr(mod, a, v)
        return False


def test_documented_switches_are_twelve_and_all_known():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "INTEGRATION.md")).read()
    table = txt[txt.index("| variable | default | effect |"):]
    table = table[:table.index("\n\n")]
    doc = set(re.findall(r"`(HPRI_[A-Z0-9_]+)`", "\n".join(ln.split("|")[1] for ln in table.splitlines()[2:])))
    assert len(doc) <= 12, sorted(doc)
    assert set(SWITCHES) <= doc, sorted(set(SWITCHES) - doc)
    # ... and every HPRI_* variable the package reads is a documented one (bench / test harness variables aside)
    src = "".join(open(os.path.join(root, "hyperpri_amd", f)).read() for f in os.listdir(os.path.join(root, "hyperpri_amd")) if f.endswith(".py"))
    read = set(re.findall(r"environ(?:\.get|\.setdefault)?\(?\[?\"(HPRI_[A-Z0-9_]+)\"", src))
    assert read <= doc, sorted(read - doc)


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
def test_pairwise_switch_matrix(prec):
    import hyperpri_amd as H
    nets = _nets()
    names = [n for n, (_, _, _, modes) in SWITCHES.items() if prec in modes]
    combos = [(n,) for n in names] + list(itertools.combinations(names, 2))
    worst = 0.0
    for kind, (net, x, m) in nets.items():
        H.set_precision(net, prec)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        lg0, g0 = _step(net, x, m, sd)
        assert torch.isfinite(lg0).all()
        for combo in combos:
            with _Set(combo):
                lg, g = _step(net, x, m, sd)
            assert torch.isfinite(lg).all(), (kind, combo)
            for (k, _), a, b in zip(net.named_parameters(), g0, g):
                assert torch.isfinite(b).all(), (kind, combo, k)
                ref = float(a.double().norm())
                if ref < 1e-6:
                    continue
                err = float((a.double() - b.double()).norm()) / ref
                worst = max(worst, err)
                assert err <= BAND[prec], (kind, combo, k, err)
    record_margin(f"switch_matrix/{prec}", worst, BAND[prec])
