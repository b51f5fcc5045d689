"""precision "torch": accepted by set_precision, and resolved from PyTorch's own settings (torch.autocast on device type "cuda",
torch.set_float32_matmul_precision) by the table of DESIGN.md ("Mixed precision").  The ambient state is set through torch's setters
(no GPU needed: ``torch.autocast("cuda")`` itself turns off without one)."""
import contextlib

import pytest
import torch


@contextlib.contextmanager
def _ambient(autocast_dtype=None, matmul="highest"):
    old = (torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda"), torch.get_float32_matmul_precision())
    try:
        if autocast_dtype is not None:
            torch.set_autocast_enabled("cuda", True)
            torch.set_autocast_dtype("cuda", autocast_dtype)
        torch.set_float32_matmul_precision(matmul)
        yield
    finally:
        torch.set_autocast_enabled("cuda", old[0])
        torch.set_autocast_dtype("cuda", old[1])
        torch.set_float32_matmul_precision(old[2])


def test_set_precision_accepts_torch():
    import hyperpri_amd as H
    net = H.set_precision(H.CubeNET(6, 1, first_depth=64, bilinear=False), "torch")
    assert all(m.hpri_precision == "torch" for m in net.modules())
    with pytest.raises(ValueError):
        H.set_precision(H.OutConv(4, 1), "fp16")


@pytest.mark.parametrize("matmul,mode", [("highest", "fp32"), ("high", "bf16x3"), ("medium", "bf16")])
def test_matmul_precision_maps_to_a_mode(matmul, mode):
    from hyperpri_amd import engine as E
    with _ambient(matmul=matmul):
        assert E.resolve_torch_precision() == mode


@pytest.mark.parametrize("dtype,mode", [(torch.float16, "f16"), (torch.bfloat16, "bf16")])
@pytest.mark.parametrize("matmul", ["highest", "high", "medium"])
def test_autocast_wins_over_matmul_precision(dtype, mode, matmul):
    from hyperpri_amd import engine as E
    with _ambient(dtype, matmul):
        assert E.resolve_torch_precision() == mode


def test_unsupported_autocast_dtype_raises():
    from hyperpri_amd import engine as E
    with _ambient(torch.float32):
        with pytest.raises(RuntimeError, match="float32"):
            E.resolve_torch_precision()


def test_modules_report_the_mode_of_the_call():
    """What the engine reads for a module: its explicit mode, or -- under "torch", also as the default (HPRI_PRECISION=torch) --
    the mode resolved for the current call; the library follows ("f16": the half-precision one)."""
    import hyperpri_amd as H
    from hyperpri_amd import engine as E
    net = H.set_precision(H.OutConv(4, 1), "torch")
    with _ambient(torch.float16):
        assert (E.precision_of(net), E.lib_kind_of(net)) == ("bf16", "f16")
    with _ambient(matmul="high"):
        assert (E.precision_of(net), E.lib_kind_of(net)) == ("bf16x3", None)
    explicit = H.set_precision(H.OutConv(4, 1), "f16")
    with _ambient(matmul="high"):
        assert (E.precision_of(explicit), E.lib_kind_of(explicit)) == ("bf16", "f16")
    plain = H.OutConv(4, 1)
    old = E.DEFAULT_PRECISION
    try:
        with _ambient(torch.bfloat16):
            assert (E.precision_of(plain), E.lib_kind_of(plain)) == (old, None)
            E.DEFAULT_PRECISION = "torch"
            assert (E.precision_of(plain), E.lib_kind_of(plain)) == ("bf16", None)
    finally:
        E.DEFAULT_PRECISION = old


def test_one_resolution_per_call():
    """Inside a call the mode resolved at its start holds, whatever the ambient state does meanwhile."""
    import hyperpri_amd as H
    from hyperpri_amd import engine as E
    net = H.set_precision(H.OutConv(4, 1), "torch")
    seen = []

    def body(module):
        seen.append(E.precision_of(module))
        torch.set_float32_matmul_precision("medium")
        seen.append(E.precision_of(module))

    with _ambient(matmul="high"):
        E.per_call_precision(body)(net)
    assert seen == ["bf16x3", "bf16x3"]


def test_f16_loss_scale_rule_is_selectable():
    from hyperpri_amd import engine as E
    assert E.F16_LOSS_SCALE == "adaptive"
