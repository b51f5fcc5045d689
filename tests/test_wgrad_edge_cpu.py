"""Plan option "wgrad_skip_edge" of the HIP library (csrc/api.cpp, option index 6): the fp32 Winograd weight gradient leaves out
the MFMA k-steps right of the image edge.  Host side only: the option is known, takes 0 and 1, and does not change the plan
(splits, slab sizes) of the benched layers -- the skip shortens strips, it never re-plans."""
import ctypes

import pytest

# CubeNET-64 on two 238x608x968 cubes: (N, H, W, Cin_pad, Cout_pad) of the 3x3 layers, one per level, and the first one
BENCHED = [(2, 608, 968, 64, 64), (2, 304, 484, 128, 128), (2, 152, 242, 256, 256), (2, 76, 121, 512, 512),
           (2, 38, 60, 1024, 1024), (2, 608, 968, 240, 64)]


@pytest.fixture()
def lib():
    from hyperpri_amd import _lib
    lib = _lib.load()
    saved = lib.hpri_get_option(b"wgrad_skip_edge")
    yield lib
    lib.hpri_set_option(b"wgrad_skip_edge", saved)


def test_option_is_known_and_defaults_to_on(lib):
    assert lib.hpri_get_option(b"wgrad_skip_edge") in (0, 1)
    for v in (0, 1):
        assert lib.hpri_set_option(b"wgrad_skip_edge", v) == 0
        assert lib.hpri_get_option(b"wgrad_skip_edge") == v
    assert lib.hpri_set_option(b"wgrad_skip_edges", 1) == -1           # an unknown name is still an error
    assert lib.hpri_set_option(b"no_such_option", 1) == -1


def test_default_is_on_unless_the_environment_says_otherwise(lib):
    import os
    if "HPRI_WGRAD_SKIP_EDGE" not in os.environ:
        assert lib.hpri_get_option(b"wgrad_skip_edge") == 1


@pytest.mark.parametrize("shape", BENCHED)
def test_plan_does_not_depend_on_the_option(lib, shape):
    N, H, W, cin_pad, cout_pad = shape
    plans = []
    for v in (0, 1):
        assert lib.hpri_set_option(b"wgrad_skip_edge", v) == 0
        sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.hpri_wino_wgrad_plan(N, H, W, cin_pad, cout_pad, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)) == 0
        plans.append((sp.value, cr.value, nr.value))
    assert plans[0] == plans[1]
    assert plans[0][0] >= 1 and plans[0][1] % 64 == 0 and plans[0][2] % 64 == 0
