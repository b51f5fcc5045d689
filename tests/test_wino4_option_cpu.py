"""Plan option "wino4_fast_epilogue" of the HIP library (csrc/api.cpp, option index 7): workgroups of the fp32 Winograd convolution
whose tile lies inside the image and whose channel block is full take an epilogue without selects.  Host side only: the option is
known, takes 0 and 1, defaults to 1, follows HPRI_WINO4_FAST_EPILOGUE, and does not change the launch plan (tiles per launch)."""
import ctypes
import os
import subprocess
import sys

import pytest

OPT = b"wino4_fast_epilogue"
# CubeNET-64 on two 238x608x968 cubes: (N, H, W) of the 3x3 layers, one per level
BENCHED = [(2, 608, 968), (2, 304, 484), (2, 152, 242), (2, 76, 121), (2, 38, 60)]


@pytest.fixture()
def lib():
    from hyperpri_amd import _lib
    lib = _lib.load()
    saved = lib.hpri_get_option(OPT)
    yield lib
    lib.hpri_set_option(OPT, saved)


def test_option_is_known_and_takes_both_values(lib):
    assert lib.hpri_get_option(OPT) in (0, 1)
    for v in (0, 1):
        assert lib.hpri_set_option(OPT, v) == 0
        assert lib.hpri_get_option(OPT) == v
    assert lib.hpri_set_option(b"wino4_fast_epilog", 1) == -1            # an unknown name is still an error
    assert lib.hpri_set_option(OPT, -1) == -1                            # and so is a negative value
    assert lib.hpri_get_option(OPT) == 1


def test_the_other_options_keep_their_values(lib):
    before = {n: lib.hpri_get_option(n) for n in (b"wgrad_skip_edge", b"wgrad_cu_reserve", b"bn_wide_cq", b"conv_nbx_min")}
    assert lib.hpri_set_option(OPT, 0) == 0
    assert {n: lib.hpri_get_option(n) for n in before} == before


def test_default_is_on_unless_the_environment_says_otherwise(lib):
    if "HPRI_WINO4_FAST_EPILOGUE" not in os.environ:
        assert lib.hpri_get_option(OPT) == 1


@pytest.mark.parametrize("env,want", [("0", 0), ("1", 1), (None, 1), ("-3", 1)])
def test_the_environment_sets_the_default(env, want):
    """A fresh process: the options are read from the environment once, at the first use (a negative value = the default)."""
    from hyperpri_amd import _lib
    e = {k: v for k, v in os.environ.items() if k != "HPRI_WINO4_FAST_EPILOGUE"}
    if env is not None:
        e["HPRI_WINO4_FAST_EPILOGUE"] = env
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.hpri_get_option.argtypes = [ctypes.c_char_p]; "
            "print(l.hpri_get_option(b'wino4_fast_epilogue'), l.hpri_get_option(b'wgrad_skip_edge'))")
    out = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH], env=e, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got, other = (int(v) for v in out.stdout.split())
    assert got == want
    if "HPRI_WGRAD_SKIP_EDGE" not in os.environ:
        assert other == 1


@pytest.mark.parametrize("shape", BENCHED)
def test_plan_does_not_depend_on_the_option(lib, shape):
    N, H, W = shape
    tiles = []
    for v in (0, 1):
        assert lib.hpri_set_option(OPT, v) == 0
        t = ctypes.c_int()
        assert lib.hpri_conv_wino4_plan(N, H, W, ctypes.byref(t)) == 0
        tiles.append(t.value)
    assert tiles[0] == tiles[1] == N * -(-H // 8) * -(-W // 16)
