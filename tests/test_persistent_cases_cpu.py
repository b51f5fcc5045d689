"""What test_gpu_persistent_items.py relies on, proven on the CPU (_persistent_cases.py): for 256, 304 and 128 compute units every
case's work list meets the predicates of its regime (some workgroups with one item more than the others, the short last band, the
queue state), every item is in exactly one list, the integer operands stay inside the exactness budget, the fp64 references are
cheap, and the ingest mirror gives the item count the kernel's source states for the benched cube.

Measured here (three_or_two at 304 CUs, the largest cases): the slowest reference is f2_rows300's (343 images of 300 rows) at
0.5 s, the ingest cubes take 0.4 s, every other case under 0.1 s; the whole file runs in 12 s."""
import time

import pytest
import torch

import _persistent_cases as PC

CASES = [(g, r) for g in PC.GEOMS for r in PC.REGIMES]


def _builder(geom):
    form = PC.GEOMS[geom]["form"]
    return PC.rows_case if form == "rows" else PC.convt_case if form == "convt" else PC.conv_case


@pytest.mark.parametrize("ncu", PC.NCUS)
@pytest.mark.parametrize("geom,regime", CASES)
def test_every_case_meets_the_predicates_of_its_regime(geom, regime, ncu):
    g = PC.GEOMS[geom]
    N, m = PC.case_mirror(geom, regime, ncu)
    ok, bad = m.regime_holds(regime)
    assert ok, (geom, regime, ncu, N, bad, m.describe())
    assert m.complete() and m.slots == 2 * ncu and m.nloc * 8 == m.slots
    c = m.counts()
    lo = 1 if regime == "two_or_one" else 2
    assert sum(1 for v in c if v == lo + 1) >= m.slots // 8          # not a token few: at least an eighth of the lists is long
    assert m.nb_count >= 2
    assert m.nb_major == (geom == "v3_c512")
    # every long list changes tile at each step; the three-block geometries change block at each step of every list as well
    steps = sum(v - 1 for v in c)
    assert m.tile_changes() == steps
    assert m.block_changes() == (steps if geom in PC.BLOCKS_CHANGE else 0), (geom, m.block_changes(), steps)
    if g["form"] == "convt":                                        # the data gradient's launch: Cin columns
        Nd, md = PC.case_mirror(geom, regime, ncu, PC.dgrad_ncols_pad(g))
        assert md.regime_holds(regime)[0] and md.nb_count >= 2
        assert Nd == N                                              # one set of images serves both directions


def test_every_kernel_has_a_case_whose_lists_change_block():
    for kernel in PC.KERNELS:
        assert any(PC.GEOMS[g]["kernel"] == kernel for g in PC.BLOCKS_CHANGE), kernel


def test_the_mirror_decodes_like_tile_of():
    """Hand-checked against the kernels' tile_of at a small launch: 3 CUs would be 0 lists, so 8 CUs = 16 slots, nloc = 2."""
    m = PC.Mirror("gemm_f32v2", 8, 21, 256)                         # 42 items, per_xcd 6: band 7 holds items 42 .. 47 = none
    assert (m.items, m.per_xcd, m.nloc, m.depth, m.queue) == (42, 6, 2, 3, True)
    assert m.lists[(0, 0)] == [(0, 0), (1, 0), (2, 0)] and m.lists[(0, 1)] == [(0, 1), (1, 1), (2, 1)]
    assert m.lists[(6, 1)] == [(18, 1), (19, 1), (20, 1)] and m.lists[(7, 0)] == [None, None, None]
    m = PC.Mirror("gemm_bf16v3", 8, 19, 256)                        # 38 items, per_xcd 5: band 7 holds items 35, 36, 37
    assert m.lists[(7, 0)] == [(17, 1), (18, 1), None] and m.lists[(7, 1)] == [(18, 0), None, None]
    assert m.absent_inside_a_band() == [(7, 0, 2), (7, 1, 1)] and m.queue and m.complete()   # per_xcd 5 >= 2 nloc
    m = PC.Mirror("conv_bf16v3", 8, 3, 1024)                        # channel-block-major: 16 blocks, band x owns blocks x and 8 + x
    assert (m.nb_major, m.per_xcd, m.nloc) == (True, 6, 2)
    assert m.lists[(5, 0)] == [(0, 5), (1, 5), (2, 5)] and m.lists[(5, 1)] == [(0, 13), (1, 13), (2, 13)] and m.complete()
    m = PC.Mirror("conv_bf16v3", 8, 5, 192)                         # banded: 15 items, per_xcd 2 = nloc
    assert (m.nb_major, m.per_xcd, m.nloc, m.queue) == (False, 2, 2, False) and m.lists[(7, 0)] == [(4, 2)] and m.lists[(7, 1)] == [None]
    m = PC.Mirror("conv_bf16v3", 8, 40, 128, ksplit=2)              # split-K halves the workgroups of a slice
    assert m.nloc == 1 and m.queue
    assert not PC.Mirror("conv_ingest", 8, 40, 128).queue           # the ingest kernel has no queue


def test_tile_tables_of_one_image():
    assert PC.gemm_tiles(5) == 1 and PC.gemm_tiles(300) == 2 and PC.gemm_tiles(256) == 1
    assert PC.v3_segments(5, 7) == ([(32, 0, 1, 0)], 1)
    assert PC.v3_segments(608, 968)[1] == 2299                      # conv_bf16v3.hip: 30 columns of 32 + one of 8: 2 images = 4598
    segs, tiles = PC.ingest_segments(9, 40)
    assert segs == [(32, 0, 1, 0), (8, 32, 1, 2)] and tiles == 3    # two 32-wide tiles of 8 rows, one 8-wide tile of 32 rows
    assert [PC.tile_in_image(segs, y, x) for y, x in ((0, 0), (7, 31), (8, 0), (0, 32), (8, 39))] == [0, 0, 1, 2, 2]
    assert PC.ingest_segments(64, 31) == ([(32, 0, 1, 0)], 8) and PC.ingest_segments(16, 44)[0] == [(32, 0, 1, 0), (16, 32, 1, 2)]


def test_the_ingest_mirror_gives_the_item_count_its_source_states():
    """conv_ingest.hip: '2 x 238x608x968: 4598 items = 8.98 rounds of 512 workgroups'."""
    tiles = PC.ingest_segments(608, 968)[1]
    m = PC.Mirror("conv_ingest", 256, 2 * tiles, 64)
    assert m.items == 4598 and m.slots == 512 and abs(m.items / m.slots - 8.98) < 0.005
    assert max(m.counts()) == 9 and min(m.counts()) == 8 and m.complete()


@pytest.mark.parametrize("ncu", PC.NCUS)
def test_operands_stay_under_the_budget_and_references_are_cheap(ncu):
    slowest = 0.0
    for geom, regime in CASES:
        g = PC.GEOMS[geom]
        N = PC.choose_images(geom, regime, ncu)
        build = _builder(geom)
        build.cache_clear()
        t0 = time.perf_counter()
        c = build(geom, N)
        slowest = max(slowest, time.perf_counter() - t0)
        assert c["budget"] < PC.LIMIT, (geom, regime, c["budget"])
        for k in ("x", "w", "wt", "dy"):
            if k in c:
                assert float(c[k].abs().max()) == 3.0 and torch.equal(c[k], c[k].round())
                assert torch.equal(c[k], c[k].to(torch.bfloat16).float()) and torch.equal(c[k], c[k].half().float())
        for k in ("bias", "y0", "dx0"):
            if k in c:
                assert float(c[k].abs().max()) == 8.0 and torch.equal(c[k], c[k].round())
        ref = c["fwd"] if "fwd" in c else c["ref"]
        assert torch.equal(ref, ref.round()) and not bool((ref == PC.SENTINEL).any())
        # images differ: no two images share their first output row (a tile computed from the wrong image is visible)
        rows = ref.reshape(N, -1)
        assert len({tuple(r[:64].tolist()) for r in rows}) == N, geom
        # tiles partition the rows
        tr = PC.tile_rows(g, N)
        assert len(tr) == N * PC.geom_tiles(g)
        npx = N * (g["HW"] if g["form"] == "rows" else g["H"] * g["W"])
        assert torch.equal(torch.cat(tr).sort().values, torch.arange(npx))
    assert slowest < 2.0, slowest


def test_first_wrong_names_the_item_and_its_list_position():
    g = PC.GEOMS["f2_rows300"]
    N, m = PC.case_mirror("f2_rows300", "three_or_two", 256)
    bad = torch.zeros(N * 300, 200, dtype=torch.bool)
    tile, block = m.lists[(3, 5)][1]
    img, tin = divmod(tile, 2)
    bad[img * 300 + tin * 256 + 7, block * 128 + 9] = True
    msg = PC.first_wrong(g, N, m, bad, "y")
    assert "image %d, tile %d of it, block %d" % (img, tin, block) in msg and "(xcd 3, j 5)" in msg and "list position 1" in msg
    assert msg.endswith("{1: 1}") and PC.first_wrong(g, N, m, torch.zeros_like(bad)) == ""
