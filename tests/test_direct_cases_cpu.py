"""CPU half of the direct-kernel tests (tests/_direct_cases.py): every integer case of the tables stays inside the 2^24 exactness
budget -- so the bit-for-bit comparisons of test_gpu_direct_conv.py / test_gpu_direct_wgrad.py are justified by the inputs, not by
the kernels --, the fp64 references agree with an index-by-index restatement, and the library's host-only plan queries show that
each geometry reaches the launch path it was chosen for (column bands, split-K, pixel-split slabs)."""
import ctypes

import pytest
import torch

import _direct_cases as D


def _fwd_opsets():
    out = [(n, "small") for n in list(D.FWD_CASES) + list(D.XCD_FWD_CASES)]
    out += [(n, o) for n in D.WIDE_FWD_CASES for o in ("a_wide", "b_wide")]
    out += [(n, o) for n in D.THIRD_FWD_CASES for o in ("a_third", "b_third")]
    return out + [(n, o) for n in D.DEEP_FWD_CASES for o in ("a_deep", "b_deep")]


def _convt_opsets():
    out = [(n, "small") for n in D.CONVT_CASES] + [(n, o) for n in D.CONVT_CASES for o in ("a_wide", "b_wide")]
    out += [(n, o) for n in D.THIRD_CONVT_CASES for o in ("a_third", "b_third")]
    return out + [(n, o) for n in D.DEEP_CONVT_CASES for o in ("a_deep", "b_deep")]


def _wgrad_opsets():
    out = [(n, "small") for n in D.WGRAD_CASES] + [(n, o) for n in D.WIDE_WGRAD_CASES for o in ("a_wide", "b_wide")]
    out += [(n, o) for n in D.THIRD_WGRAD_CASES for o in ("a_third", "b_third")]
    return out + [(n, o) for n in D.DEEP_WGRAD_CASES for o in ("a_deep", "b_deep")]


@pytest.mark.parametrize("name,opset", _fwd_opsets())
def test_forward_cases_stay_inside_the_exactness_budget(name, opset):
    i = D.fwd_inputs(name, opset)
    assert D.fwd_budget(i["x"], i["w"], i["bias"], i["y0"]) < D.LIMIT
    for t in i.values():
        assert torch.equal(t, t.round())
    if opset == "small":                                     # every value is bf16-exact
        assert torch.equal(i["x"], i["x"].bfloat16().float()) and torch.equal(i["w"], i["w"].bfloat16().float())
    if opset.endswith("_wide"):                              # two bf16 planes hold the wide operand, one the narrow one
        for t in (i["x"], i["w"]):
            hi = t.bfloat16().float()
            assert torch.equal(hi + (t - hi).bfloat16().float(), t)
        narrow = i["w"] if opset == "a_wide" else i["x"]
        assert torch.equal(narrow, narrow.bfloat16().float())
        assert not torch.equal(i["x" if opset == "a_wide" else "w"], i["x" if opset == "a_wide" else "w"].bfloat16().float())
    if opset.endswith(("_third", "_deep")):
        t = i["x"] if opset.startswith("a_") else i["w"]
        hi = t.bfloat16().float()
        mid = (t - hi).bfloat16().float()
        lo = (t - hi - mid).bfloat16().float()
        assert torch.equal(hi + mid + lo, t) and not torch.equal(hi, t)
        # signed round-to-nearest planes: two hold every integer below 2^17; the deep set does put values into the third
        assert torch.equal(hi + mid, t) == opset.endswith("_third")


@pytest.mark.parametrize("name,opset", _convt_opsets())
def test_transposed_cases_stay_inside_the_exactness_budget(name, opset):
    c = D.CONVT_CASES[name]
    N, H, W, Cin, Cup = c["shape"]
    i = D.convt_inputs(name, opset)
    assert D.convt_budget(i["x"], i["wt"], i["bias"]) < D.LIMIT
    if opset.endswith("_deep"):
        return                                               # forward only (tests/_direct_cases.py: DEEP_CONVT_CASES)
    bdx, _ = D.convt_grad_budgets(i["x"], i["wt"], D.convt_patch(i["dy_d"], H, W, c["py0"], c["px0"]), dx0=i["dx0"])
    _, bdw = D.convt_grad_budgets(i["x"], i["wt"], D.convt_patch(i["dy_w"], H, W, c["py0"], c["px0"]), dw0=i["dw0"])
    assert bdx < D.LIMIT and bdw < D.LIMIT
    assert 2 * H + c["py0"] <= c["H2"] and 2 * W + c["px0"] <= c["W2"]
    assert (2 * H, 2 * W) != (c["H2"], c["W2"])              # there is a border that must keep its sentinel


@pytest.mark.parametrize("name,opset", _wgrad_opsets())
def test_weight_gradient_cases_stay_inside_the_exactness_budget(name, opset):
    i = D.wgrad_inputs(name, opset)
    assert D.wgrad_budget(i["x"], i["dy"], D.WGRAD_CASES[name]["ks"], i["dw0"]) < D.LIMIT


def test_references_agree_with_an_index_by_index_restatement():
    i = D.fwd_inputs("plain_odd_two_images", random=True)
    assert float((D.ref_conv(i["x"], i["w"], i["bias"]) - D.naive_conv(i["x"], i["w"], i["bias"])).abs().max()) < 1e-12
    i = D.fwd_inputs("k1_no_split")
    assert torch.equal(D.ref_conv(i["x"], i["w"], i["bias"]), D.naive_conv(i["x"], i["w"], i["bias"]))     # integers: exactly
    g = D.wgrad_inputs("cvalid_8", random=True)
    assert float((D.ref_wgrad(g["x"], g["dy"], 3) - D.naive_wgrad(g["x"], g["dy"], 3)).abs().max()) < 1e-11
    g = D.wgrad_inputs("k1_wide_rows")
    assert torch.equal(D.ref_wgrad(g["x"], g["dy"], 1), D.naive_wgrad(g["x"], g["dy"], 1))
    c = D.CONVT_CASES["convt_cup8_off10"]
    N, H, W, Cin, Cup = c["shape"]
    t = D.convt_inputs("convt_cup8_off10", random=True)
    assert float((D.ref_convt(t["x"], t["wt"], t["bias"]) - D.naive_convt(t["x"], t["wt"], t["bias"])).abs().max()) < 1e-12
    # the transposed convolution's gradients: dx = the forward's adjoint, dw[ci][co][a][b] = sum x[.., ci] dy[2y+a, 2x+b, co]
    dyp = D.convt_patch(t["dy_d"], H, W, c["py0"], c["px0"])
    dx, dw = D.ref_convt_grads(t["x"], t["wt"], dyp)
    want_dx = torch.zeros(N, H, W, Cin, dtype=torch.float64)
    want_dw = torch.zeros(Cin, Cup, 2, 2, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            want_dx += dyp[:, a::2, b::2].double() @ t["wt"][:, :, a, b].double().t()
            want_dw[:, :, a, b] = t["x"].double().reshape(-1, Cin).t() @ dyp[:, a::2, b::2].double().reshape(-1, Cup)
    assert float((dx - want_dx.reshape(-1, Cin)).abs().max()) < 1e-12 and float((dw - want_dw).abs().max()) < 1e-11


def test_pack_restatement_matches_the_documented_layouts():
    """pack_expected against the layouts written out with tensor indexing: mode 0 wp[t][k][n] = W[n][k][t], mode 1
    wp[t][k = n][col = c] = W[n][c][T-1-t], mode 2 wp[0][ci][tap*Cup + co] = Wt[ci][co][tap], mode 3 its transpose."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(7, 5, 3, 3, generator=g)
    e0 = D.pack_expected(w, 0, 5, 7, 64, 9, 5, 0)
    assert e0.shape == (1, 9, 32, 64)
    assert torch.equal(torch.from_numpy(e0[0, :, :5, :7]), w.reshape(7, 5, 9).permute(2, 1, 0))
    e1 = D.pack_expected(w, 1, 7, 5, 64, 9, 5, 0)
    assert torch.equal(torch.from_numpy(e1[0, :, :7, :5]), w.reshape(7, 5, 9).flip(2).permute(2, 0, 1))
    wt = torch.randn(5, 4, 2, 2, generator=g)
    e2 = D.pack_expected(wt, 2, 5, 16, 64, 1, 0, 4)
    assert torch.equal(torch.from_numpy(e2[0, 0, :5, :16]), wt.reshape(5, 4, 4).permute(0, 2, 1).reshape(5, 16))
    e3 = D.pack_expected(wt, 3, 16, 5, 64, 1, 0, 4)
    assert torch.equal(torch.from_numpy(e3[0, 0, :16, :5]), torch.from_numpy(e2[0, 0, :5, :16]).t())
    assert float(abs(e0[0, :, 5:, :]).max()) == 0.0 and float(abs(e0[0, :, :, 7:]).max()) == 0.0


@pytest.fixture(scope="module")
def lib():
    from hyperpri_amd import _lib
    return _lib.load()


def _fwd_plan(lib, N, H, W, cin_pad, cout_pad, ks, amode=0, epi=0, split=None):
    k, t, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    if split is None:
        assert lib.hpri_conv_fwd_plan(N, H, W, cin_pad, cout_pad, ks, amode, epi, ctypes.byref(k), ctypes.byref(t), ctypes.byref(w)) == 0
    else:
        assert lib.hpri_conv_fwd_bf16_plan(N, H, W, cin_pad, cout_pad, ks, amode, epi, split, ctypes.byref(k), ctypes.byref(t), ctypes.byref(w)) == 0
    return k.value, t.value, w.value


def test_plan_arithmetic_of_the_cases(lib):
    """The plan queries are host-only, so what each geometry reaches is known without a GPU: column bands (stat_tiles differs from
    the plain count), split-K factors with uneven chunk splits and a partial last chunk, pixel-split slabs, the reduce kernel."""
    for name, c in D.FWD_CASES.items():
        N, H, W, Cin, Cout = c["shape"]
        cin_pad, cout_pad = D.rup(Cin, 8), D.rup(Cout, 64)
        k, tiles, wsf = _fwd_plan(lib, N, H, W, cin_pad, cout_pad, c["ks"])
        if c["ksplit"] is not None:
            assert k == c["ksplit"], (name, k)
        if k > 1:
            assert tiles == N * D.cdiv(H * W, 64) and wsf == k * N * H * W * cout_pad
            chunks = D.cdiv(cin_pad, 32)
            assert chunks % k != 0 or cin_pad % 32 != 0, name          # uneven chunk split or a partial last chunk
        else:
            assert wsf == 0
        if c["seg"] is True:
            assert tiles != D.plain_tiles(N, H, W, cout_pad), name
        if c["seg"] is False:
            assert tiles == D.plain_tiles(N, H, W, cout_pad), name
        if "tiles" in c:
            assert tiles == c["tiles"]
    assert D.FWD_CASES["splitk2_partial_chunk"]["shape"][3] % 32 == 4             # 260: nine chunks, the ninth holds 8 of 32 channels
    # both workgroup shapes, and the narrow bf16x6 one, meet bands somewhere
    N, H, W, Cin, Cout = D.FWD_CASES["4x1_bands_32_8"]["shape"]
    assert _fwd_plan(lib, N, H, W, 8, 64, 3, split=2)[1] != D.plain_tiles(N, H, W, 64, narrow=True)
    assert _fwd_plan(lib, N, H, W, 8, 64, 3, split=1)[1] != D.plain_tiles(N, H, W, 64)
    for name, c in D.XCD_FWD_CASES.items():
        N, H, W, Cin, Cout = c["shape"]
        k, tiles, _ = _fwd_plan(lib, N, H, W, D.rup(Cin, 8), D.rup(Cout, 64), c["ks"])
        nb = D.rup(Cout, 64) // (128 if D.rup(Cout, 64) % 128 == 0 else 64)
        assert k == 1 and tiles % 8 != 0 and nb >= 2, name              # 1-D grid with blocks that return early
    sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for name, c in D.WGRAD_CASES.items():
        N, H, W, Cin, Cout = c["shape"]
        assert lib.hpri_wgrad_plan(N, H, W, D.rup(Cin, 8), D.rup(Cout, 64), c["ks"], ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)) == 0
        strips = N * D.cdiv(H, 2) * D.cdiv(W, 32)
        assert 1 <= sp.value <= strips and (sp.value > 1 or strips == 1), name
    assert lib.hpri_wgrad_plan(1, 9, 40, 72, 192, 3, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)) == 0
    assert (cr.value // 64, nr.value // 64) == (2, 3)
    assert lib.hpri_wgrad_plan(1, 7, 13, 136, 128, 1, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)) == 0
    assert (cr.value // 128, nr.value // 128) == (2, 1)
    assert lib.hpri_wgrad_plan(1, 3, 9, 16, 192, 1, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)) == 0
    assert (cr.value // 128, nr.value // 128) == (1, 2)
    # ConvTranspose2d weight gradients: Cup 32 with <= 16 slabs takes wgrad_reduce_convt_kernel, Cup 8 the generic reduce
    for name, c in D.CONVT_CASES.items():
        N, H, W, Cin, Cup = c["shape"]
        assert lib.hpri_wgrad_plan(N, H, W, D.rup(Cin, 8), D.rup(4 * Cup, 64), 1, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)) == 0
        assert 1 < sp.value <= 16
    assert D.CONVT_CASES["convt_cup32"]["shape"][4] % 16 == 0 and D.CONVT_CASES["convt_cup8_off01"]["shape"][4] % 16 != 0
    # the XCD-aware weight-gradient grid: 8k slabs over 10 strips, so most slabs are empty
    saved = [lib.hpri_get_option(o) for o in (b"wgrad_xcd_min_tiles", b"wgrad_xcd_min_strips")]
    try:
        assert lib.hpri_set_option(b"wgrad_xcd_min_tiles", 1) == 0 and lib.hpri_set_option(b"wgrad_xcd_min_strips", 1) == 0
        assert lib.hpri_wgrad_plan(1, 9, 40, 72, 192, 3, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)) == 0
        assert sp.value % 8 == 0 and sp.value > 1 * D.cdiv(9, 2) * D.cdiv(40, 32)
    finally:
        lib.hpri_set_option(b"wgrad_xcd_min_tiles", saved[0])
        lib.hpri_set_option(b"wgrad_xcd_min_strips", saved[1])
