"""``hyperpri_amd.cache.plan_batch`` -- the host half of ``CubeCache.batch``: per-sample normalisation, validation, the choice between
the plain gather, the warp pair and the deforming kernels, and the host tensors each path uploads.  Pure host logic: no GPU, no
library."""
import numpy as np
import pytest
import torch

from hyperpri_amd.cache import deform_entries, elastic_lattice, plan_batch, warp_entries

FRAME, C = (40, 60), 7
IDX = [2, 0, 1]
WIN = dict(patch=(16, 24), top=[3, 0, 24], left=[5, 36, 0], flip_h=[0, 1, 1], flip_w=[1, 0, 1])
NEUTRAL = dict(angle=0.0, zoom=[1.0, 1.0, 1.0], shift=(0.0, 0.0), gain=1, offset=[0, 0, 0], band_drop=(3, 0), noise=(0.0, 7, 9),
               cutmix=(-1, 0, 8, 0, 8))


def _plan(**kw):
    return plan_batch(IDX, FRAME, C, **dict(WIN, **kw))


def _warp_rows(**kw):
    v = dict(angle=[0.0] * 3, zoom=[1.0] * 3, sx=[0.0] * 3, sy=[0.0] * 3, gain=[1.0] * 3, offset=[0.0] * 3, lo=[0] * 3, n=[0] * 3)
    v.update(kw)
    return warp_entries(IDX, WIN["top"], WIN["left"], WIN["flip_h"], WIN["flip_w"], (16, 24), v["angle"], v["zoom"], v["sx"], v["sy"],
                        v["gain"], v["offset"], v["lo"], v["n"])


def _deform_rows(mix=((-1, 0, 0, 0, 0),) * 3, off=(-1,) * 3, gy=0, gx=0, inv_pitch=0.0, sigma=(0.0,) * 3, k0=(0,) * 3, k1=(0,) * 3):
    return deform_entries(*[[m[c] for m in mix] for c in range(5)], list(off), [gy] * 3, [gx] * 3, [inv_pitch] * 3, list(sigma), list(k0),
                          list(k1))


def test_neutral_values_give_the_gather_table():
    want = torch.tensor([[2, 3, 5, 2], [0, 0, 36, 1], [1, 24, 0, 3]], dtype=torch.int32)        # {slot, top, left, flip_h | 2 flip_w}
    for kw in ({}, NEUTRAL):
        p = _plan(**kw)
        assert p.path == "gather" and p.window == (16, 24)
        assert p.table.dtype == torch.int32 and torch.equal(p.table, want)
        assert p.entries is None and p.deform is None and p.nodes is None
    p = plan_batch([4, 1], FRAME, C)                                    # the whole frame, nothing given
    assert p.path == "gather" and p.window == FRAME and p.table.tolist() == [[4, 0, 0, 0], [1, 0, 0, 0]]
    p = plan_batch([4], FRAME, C, patch=10)                             # a smaller window is centred
    assert p.table.tolist() == [[4, 15, 25, 0]]


@pytest.mark.parametrize("kw, rows", [
    (dict(angle=[0.0, 12.5, 0.0]), dict(angle=[0.0, 12.5, 0.0])),
    (dict(angle=90.0), dict(angle=[90.0] * 3)),
    (dict(zoom=[1.0, 1.0, 0.75]), dict(zoom=[1.0, 1.0, 0.75])),
    (dict(shift=[(0.0, 0.0), (0.0, -1.5), (0.25, 0.0)]), dict(sx=[0.0, 0.0, 0.25], sy=[0.0, -1.5, 0.0])),
    (dict(gain=1.1), dict(gain=[1.1] * 3)),
    (dict(offset=[0.0, 0.0, -0.2]), dict(offset=[0.0, 0.0, -0.2])),
    (dict(band_drop=[(0, 0), (2, 3), (0, 0)]), dict(lo=[0, 2, 0], n=[0, 3, 0])),
    (dict(angle=-33.0, zoom=1.25, shift=(0.5, 0.25), gain=[0.8, 1.0, 1.3], offset=0.1, band_drop=(6, 1)),
     dict(angle=[-33.0] * 3, zoom=[1.25] * 3, sx=[0.5] * 3, sy=[0.25] * 3, gain=[0.8, 1.0, 1.3], offset=[0.1] * 3, lo=[6] * 3, n=[1] * 3)),
])
def test_any_non_neutral_value_gives_the_warp_entries(kw, rows):
    p = _plan(**kw)
    assert p.path == "warp" and p.window == (16, 24)
    assert p.entries.dtype == torch.int32 and torch.equal(p.entries, _warp_rows(**rows))
    assert p.table is None and p.deform is None and p.nodes is None


def test_forcing_a_path_keeps_the_neutral_entries():
    p = _plan(force_warp=True)
    assert p.path == "warp" and torch.equal(p.entries, _warp_rows())
    p = _plan(force_deform=True)
    assert p.path == "deform" and torch.equal(p.entries, _warp_rows()) and torch.equal(p.deform, _deform_rows()) and p.nodes is None


def test_elastic_noise_or_a_partner_inside_the_batch_give_the_deform_entries():
    gy, gx = elastic_lattice(16, 24, 8.0)
    nodes = np.random.default_rng(3).normal(size=(3, gy, gx, 2)) * 2.0
    p = _plan(elastic=(nodes, 8.0))
    assert p.path == "deform" and torch.equal(p.entries, _warp_rows())
    cell = 2 * gy * gx
    assert p.deform[:, 5].tolist() == [0, cell, 2 * cell]                                       # nodes_off = j * 2 gy gx
    assert torch.equal(p.deform, _deform_rows(off=(0, cell, 2 * cell), gy=gy, gx=gx, inv_pitch=1 / 8.0))
    assert p.nodes.dtype == torch.float32 and p.nodes.shape == (3 * cell,)
    assert torch.equal(p.nodes, torch.from_numpy(nodes).to(torch.float32).reshape(-1))
    assert p.table is None

    p = _plan(noise=[(0.0, 1, 2), (0.05, 2 ** 32 - 1, 0), (0.0, 5, 6)])
    assert p.path == "deform" and p.nodes is None and torch.equal(p.entries, _warp_rows())
    assert torch.equal(p.deform, _deform_rows(sigma=(0.0, 0.05, 0.0), k0=(1, 2 ** 32 - 1, 5), k1=(2, 0, 6)))
    assert (p.deform[:, 5] == -1).all()

    mix = [(-1, 0, 0, 0, 0), (0, 2, 9, -4, 30), (-1, 0, 0, 0, 0)]                               # (the kernels clamp the rectangle)
    p = _plan(cutmix=mix)
    assert p.path == "deform" and torch.equal(p.deform, _deform_rows(mix=mix))

    # all three on top of a warp: the warp entries are those of the warp path
    kw = dict(angle=17.0, zoom=0.8, gain=[1.0, 1.2, 1.0], band_drop=(1, 2))
    p = _plan(elastic=(nodes, 8.0), noise=(0.1, 11, 12), cutmix=[(2, 0, 8, 0, 8), (-1, 0, 0, 0, 0), (1, 4, 16, 12, 24)], **kw)
    assert p.path == "deform" and torch.equal(p.entries, _plan(**kw).entries)
    assert torch.equal(p.deform, _deform_rows(mix=[(2, 0, 8, 0, 8), (-1, 0, 0, 0, 0), (1, 4, 16, 12, 24)], off=(0, cell, 2 * cell), gy=gy, gx=gx,
                                              inv_pitch=1 / 8.0, sigma=(0.1,) * 3, k0=(11,) * 3, k1=(12,) * 3))


def _mix(rect, partner=lambda j: (j + 1) % 3):
    return [(partner(j),) + rect for j in range(3)]


@pytest.mark.parametrize("mix", [
    _mix((0, 8, 0, 8), lambda j: j),                                                            # from the sample itself
    _mix((0, 8, 0, 8), lambda j: 3), _mix((0, 8, 0, 8), lambda j: -1), _mix((0, 8, 0, 8), lambda j: -7),      # from outside the batch
    _mix((5, 5, 0, 8)), _mix((0, 8, 9, 3)),                                                     # an empty rectangle
    _mix((-6, 0, 0, 8)), _mix((16, 20, 0, 8)), _mix((0, 8, 24, 40)), _mix((0, 8, -3, 0)),       # empty once clamped into 16 x 24
])
def test_a_cutmix_that_mixes_nothing_does_not_select_the_deform_path(mix):
    assert _plan(cutmix=mix).path == "gather"
    p = _plan(cutmix=mix, gain=1.5)
    assert p.path == "warp" and torch.equal(p.entries, _warp_rows(gain=[1.5] * 3))
    assert _plan(cutmix=_mix((0, 8, 0, 8))).path == "deform"                                    # (the same rectangle from a partner)


def test_validation_errors_keep_their_texts():
    with pytest.raises(ValueError, match=r"CubeCache.batch: no indices"):
        plan_batch([], FRAME, C)
    with pytest.raises(ValueError, match=r"CubeCache: a 41x60 window does not fit a 40x60 frame"):
        plan_batch(IDX, FRAME, C, patch=(41, 60))
    with pytest.raises(ValueError, match=r"CubeCache.batch: window 16x24 at \(25, 0\) leaves the 40x60 frame"):
        _plan(top=[3, 0, 25])
    with pytest.raises(ValueError, match=r"CubeCache.batch: window 16x24 at \(3, -1\) leaves the 40x60 frame"):
        _plan(left=[-1, 36, 0])
    with pytest.raises(ValueError, match=r"CubeCache.batch: one value per sample"):
        _plan(top=[1, 2])
    with pytest.raises(ValueError, match=r"CubeCache.batch: one finite value per sample"):
        _plan(angle=[0.0, float("nan"), 0.0])
    with pytest.raises(ValueError, match=r"CubeCache.batch: one finite 2-tuple per sample"):
        _plan(shift=[(0.0, 0.0)] * 2)
    for z in (0.05, 16.5):
        with pytest.raises(ValueError, match=r"CubeCache.batch: zoom must lie in \[1/16, 16\]"):
            _plan(zoom=[1.0, z, 1.0])
    for d in ((5, 3), (-1, 2), (0.5, 1), (0, 1.5)):
        with pytest.raises(ValueError, match=r"CubeCache.batch: band_drop .* leaves the 7 bands"):
            _plan(band_drop=d)
    for k in ((0.1, -1, 0), (0.1, 0, 2 ** 32), (0.0, 0.5, 0)):
        with pytest.raises(ValueError, match=r"CubeCache.batch: noise keys must be whole numbers in \[0, 2\^32\)"):
            _plan(noise=k)
    for c in ((0.5, 0, 8, 0, 8), (1, 0, 8, 0, 2 ** 31)):
        with pytest.raises(ValueError, match=r"CubeCache.batch: cutmix takes whole numbers \(from, ry0, ry1, rx0, rx1\)"):
            _plan(cutmix=c)
    gy, gx = elastic_lattice(16, 24, 8.0)
    with pytest.raises(ValueError, match=rf"CubeCache.batch: a 16x24 window at pitch 8.0 needs a lattice of \({gy}, {gx}\), got \({gy + 1}, {gx}\)"):
        _plan(elastic=(np.zeros((3, gy + 1, gx, 2)), 8.0))
    for nodes, pitch in ((np.zeros((2, gy, gx, 2)), 8.0), (np.zeros((3, gy, gx, 3)), 8.0), (np.zeros((3, gy, gx, 2)), 3.0),
                         (np.full((3, gy, gx, 2), np.inf), 8.0)):
        with pytest.raises(ValueError, match=r"CubeCache.batch: elastic takes \(\(n, gy, gx, 2\) finite node displacements, pitch >= 4\)"):
            _plan(elastic=(nodes, pitch))
