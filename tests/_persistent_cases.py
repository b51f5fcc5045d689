"""Work-list mirrors, case tables, input builders and fp64 references shared by test_persistent_cases_cpu.py and
test_gpu_persistent_items.py: the second and later work items of the four persistent kernels (csrc/gemm_f32v2.hip,
csrc/gemm_bf16v3.hip, csrc/conv_bf16v3.hip, csrc/conv_ingest.hip), called through the C ABI.  ``_Queue`` (a caller-owned item queue on
a private stream) lives here too, for test_gpu_item_queue.py and test_gpu_persistent_items.py.

Everything but ``_Queue`` runs on the CPU.  A persistent launch has 2 x CUs workgroup slots (S), workgroup id mod 8 names the band
(XCD) whose items it walks, and workgroup j of a band takes items k = j, j + nloc, ... of it (nloc = S / 8).  ``mirror`` restates
that arithmetic from the launchers (f2_launch, g3_launch, v3_launch, hpri_conv3x3_ingest_h16) and the kernels' ``tile_of``, so a
case can PROVE which workgroups take a second or third item, and a failing output element can be named by the workgroup and list
position that owns it.

Regimes (functions of the CU count, because S is): ``two_or_one``: S < items < 2 S -- some workgroups take two items, some one; in
the banded orders items % 8 != 0, so the last band is short and a second item of it is absent although k < per_xcd; a registered
queue is NOT taken.  ``three_or_two``: 2 S < items < 3 S, items % 8 != 0 in the banded orders -- three items or two; a registered
queue IS taken (never by the ingest kernel, which has no queue).  The channel-block-major order of conv_bf16v3 (Cout_pad % 512 ==
0) has items = 8 x per_xcd by construction: there ``per_xcd % nloc != 0`` takes the place of ``items % 8 != 0`` (the lists of one
band have two lengths, and the absent item is the one at k >= per_xcd).

Many tiny images make many items: an image is one to three (partial) tiles, so 1300 items are a few hundred kilobytes.

Integer operands (the argument is in _direct_cases.py): both operands integers in [-3, 3] -- exact in bf16 and IEEE half --, bias
and prior output contents integers in [-8, 8], so that every partial sum is an integer below 2^24 and the result does not depend on
the summation order: fp32 outputs must equal the fp64 reference bit for bit, 16-bit outputs the exact integer rounded once."""
import ctypes
import functools

import torch

from _direct_cases import LIMIT, SENTINEL, X_PAD_VALUE, cdiv, rup, _ints

__all__ = ["LIMIT", "SENTINEL", "X_PAD_VALUE", "cdiv", "rup"]

REGIMES = ("two_or_one", "three_or_two")
NCUS = (256, 304, 128)                       # MI355X, MI300X-class, half a device: what the CPU test proves the cases for
Q_SLICES = 8                                 # common.h HPRI_Q_SLICES


# ---------------------------------------------------------------------------------------------------------------------------
# Tiles of one image, per kernel: a list of column bands (tile width, first column, tile columns, first tile index) + tile count
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_tiles(HW):
    """gemm_f32v2 / gemm_bf16v3: 256 consecutive rows of one image."""
    return cdiv(HW, 256)


def v3_segments(H, W):
    """conv_bf16v3.hip v3_segments with plan option bf16v3_tile_width = 0: n32 columns of 32-wide tiles, the rest 16 wide, a last
    remainder of at most 8 columns as one 8-wide column; cheapest padding wins, ties go to the plan without narrow tiles."""
    th = lambda tw: 256 // tw
    slots = lambda tw, ntx: cdiv(H, th(tw)) * th(tw) * tw * ntx
    best, best_cost = None, -1
    for n32 in range(cdiv(W, 32) + 1):
        rem = W - n32 * 32
        n16, n8 = (cdiv(rem, 16) if rem > 0 else 0), 0
        if rem <= 0 and n32 * 32 - W >= 32:
            continue
        if n16 > 0 and rem - (n16 - 1) * 16 <= 8:
            n16, n8 = n16 - 1, 1
        cost = (slots(32, n32) if n32 else 0) + (slots(16, n16) if n16 else 0) + (slots(8, n8) if n8 else 0)
        if best_cost < 0 or cost < best_cost or (cost == best_cost and n16 + n8 == 0):
            segs = []
            if n32:
                segs.append([32, 0, n32])
            if n16:
                segs.append([16, n32 * 32, n16])
            if n8:
                segs.append([8, n32 * 32 + n16 * 16, 1])
            best, best_cost = segs, cost
    first = 0
    for s in best:
        s.append(first)
        first += cdiv(H, th(s[0])) * s[2]
    return [tuple(s) for s in best], first


def ingest_segments(H, W):
    """hpri_conv3x3_ingest_h16: 32-wide tiles of 8 rows, and what W mod 32 leaves over (at most 16 columns) as one column of 8-wide
    (32 rows) or 16-wide (16 rows) tiles."""
    rem = W % 32
    n32 = cdiv(W, 32) if rem > 16 else W // 32
    segs, first = [], 0
    if n32 > 0:
        segs.append((32, 0, n32, first))
        first += n32 * cdiv(H, 8)
    if 0 < rem <= 16:
        tw = 8 if rem <= 8 else 16
        segs.append((tw, n32 * 32, 1, first))
        first += cdiv(H, 256 // tw)
    return segs, first


def tile_in_image(segs, y, x):
    """Index (within its image) of the tile that holds pixel (y, x)."""
    for tw, xbeg, ntx, first in segs:
        if xbeg <= x < xbeg + ntx * tw:
            return first + (y // (256 // tw)) * ntx + (x - xbeg) // tw
    raise AssertionError((segs, y, x))


# ---------------------------------------------------------------------------------------------------------------------------
# The work-list mirror
# ---------------------------------------------------------------------------------------------------------------------------
KERNELS = ("gemm_f32v2", "gemm_bf16v3", "conv_bf16v3", "conv_ingest")
BLOCK = {"gemm_f32v2": 128, "gemm_bf16v3": 128, "conv_bf16v3": 64, "conv_ingest": 64}       # columns / channels per item


class Mirror:
    """The work list of one launch: ``lists[(xcd, j)]`` = the fixed list of workgroup j of band xcd, one entry per list position
    k = j + pos * nloc: (tile, block), or None where the kernel's tile_of refuses k (beyond the band, beyond the last item)."""

    def __init__(self, kernel, ncu, ntiles, ncols_pad, ksplit=1):
        assert kernel in KERNELS
        self.kernel, self.ncu, self.ntiles = kernel, ncu, ntiles
        self.slots = 2 * ncu
        self.nb_count = cdiv(ncols_pad, BLOCK[kernel])
        self.items = ntiles * self.nb_count
        self.nb_major = kernel == "conv_bf16v3" and self.nb_count % 8 == 0
        self.per_xcd = ntiles * (self.nb_count // 8) if self.nb_major else cdiv(self.items, 8)
        self.nloc = max(1, (2 * ncu // ksplit) // 8)
        self.nloc = min(self.nloc, self.per_xcd)
        self.depth = cdiv(self.per_xcd, self.nloc)
        # f2_launch / g3_launch: per_xcd >= 2 nloc; v3_launch: also ksplit <= HPRI_Q_SLICES (and the queue's counters are per K
        # slice); the ingest kernel has no queue
        self.queue = kernel != "conv_ingest" and self.per_xcd >= 2 * self.nloc and ksplit <= Q_SLICES
        self.lists, self.owner = {}, {}
        for xcd in range(8):
            for j in range(self.nloc):
                lst = []
                for pos in range(self.depth):
                    it = self.decode(xcd, j + pos * self.nloc)
                    lst.append(it)
                    if it is not None:
                        assert it not in self.owner, it
                        self.owner[it] = (xcd, j, pos)
                self.lists[(xcd, j)] = lst

    def decode(self, xcd, k):
        """tile_of: list index k of band xcd -> (tile, block) or None."""
        if k >= self.per_xcd:
            return None
        if self.nb_major:
            nbx = self.nb_count >> 3
            bx = k // nbx
            return None if bx >= self.ntiles else (bx, (k - bx * nbx) * 8 + xcd)
        item = xcd * self.per_xcd + k
        return None if item >= self.items else divmod(item, self.nb_count)

    def counts(self):
        """Items per workgroup, over all workgroups."""
        return [sum(it is not None for it in lst) for lst in self.lists.values()]

    def absent_inside_a_band(self):
        """List positions k < per_xcd of the last band that hold no item (the band tail: items % 8 != 0)."""
        return [(7, j, pos) for j in range(self.nloc) for pos in range(self.depth)
                if j + pos * self.nloc < self.per_xcd and self.lists[(7, j)][pos] is None]

    def block_changes(self):
        """Number of list steps (an item and the next one of the same workgroup) that change the column / channel block."""
        return sum(1 for lst in self.lists.values() for a, b in zip(lst, lst[1:]) if a is not None and b is not None and a[1] != b[1])

    def tile_changes(self):
        """... that change the tile within the image (``tiles`` per image): the geometry handed over differs."""
        return sum(1 for lst in self.lists.values() for a, b in zip(lst, lst[1:]) if a is not None and b is not None and a[0] != b[0])

    def complete(self):
        return len(self.owner) == self.items and set(self.owner) == {(t, b) for t in range(self.ntiles) for b in range(self.nb_count)}

    def regime_holds(self, regime):
        """The predicates a case of ``regime`` relies on, as (ok, what failed)."""
        S, c = self.slots, self.counts()
        lo = 1 if regime == "two_or_one" else 2
        checks = {
            "every item is in exactly one list": self.complete(),
            "items between %d and %d slots" % (lo, lo + 1): lo * S < self.items < (lo + 1) * S,
            "lists of %d and %d items" % (lo + 1, lo): max(c) == lo + 1 and min(c) == lo and len(c) == S,
            "queue": self.queue == (regime == "three_or_two" and self.kernel != "conv_ingest"),
        }
        if self.nb_major:
            checks["per_xcd % nloc != 0"] = self.per_xcd % self.nloc != 0
        else:
            checks["items % 8 != 0"] = self.items % 8 != 0
            checks["an item of the last band is absent inside the band"] = len(self.absent_inside_a_band()) > 0
        bad = [k for k, v in checks.items() if not v]
        return not bad, bad

    def describe(self):
        c = self.counts()
        return dict(items=self.items, per_xcd=self.per_xcd, nloc=self.nloc, nb_major=int(self.nb_major), queue=int(self.queue),
                    block_changes=self.block_changes(), most=max(c), least=min(c), with_most=sum(1 for v in c if v == max(c)))

    def where(self, tile, block):
        xcd, j, pos = self.owner[(tile, block)]
        return "workgroup (xcd %d, j %d) = block id %d, list position %d (k = %d)" % (xcd, j, j * 8 + xcd, pos, j + pos * self.nloc)


# ---------------------------------------------------------------------------------------------------------------------------
# Case table.  A geometry fixes one image and the column blocks; N follows from the CU count and the regime.
#   kernel     which mirror
#   tiles      tiles of one image (the GPU test compares it with the library's plan query where there is one)
#   ncols_pad  packed column / channel count of the launch
# ---------------------------------------------------------------------------------------------------------------------------
GEOMS = {
    # row GEMMs: HW rows per image, K -> 200 columns = one full block of 128 + one of 72
    "f2_rows5": dict(kernel="gemm_f32v2", form="rows", HW=5, K=40, C=200, ncols_pad=256),
    "f2_rows300": dict(kernel="gemm_f32v2", form="rows", HW=300, K=40, C=200, ncols_pad=256),       # two tiles, the second with 44 rows
    "f2_rows5_b3": dict(kernel="gemm_f32v2", form="rows", HW=5, K=40, C=300, ncols_pad=320),        # three blocks, the last of the pack half there
    # ConvTranspose2d(k=2, s=2) on a 2 x 3 grid: forward 4 * Cup = 320 columns, data gradient Cin = 264 columns (Cin_pad 320)
    "f2_convt": dict(kernel="gemm_f32v2", form="convt", H=2, W=3, Cin=264, Cup=80, ncols_pad=320),
    "g3_rows5": dict(kernel="gemm_bf16v3", form="rows", HW=5, K=40, C=200, ncols_pad=256),
    "g3_rows300": dict(kernel="gemm_bf16v3", form="rows", HW=300, K=40, C=200, ncols_pad=256),
    "g3_rows5_b3": dict(kernel="gemm_bf16v3", form="rows", HW=5, K=40, C=300, ncols_pad=320),
    "g3_convt": dict(kernel="gemm_bf16v3", form="convt", H=2, W=3, Cin=264, Cup=96, ncols_pad=384),  # dgrad: Cin_pad 320, three blocks too
    # 3x3 convolutions over 5 x 7 images (one partial tile each)
    "v3_c72": dict(kernel="conv_bf16v3", form="conv", H=5, W=7, Cin=40, Cout=72, ncols_pad=128),
    "v3_c128": dict(kernel="conv_bf16v3", form="conv", H=5, W=7, Cin=40, Cout=128, ncols_pad=128),
    "v3_c136": dict(kernel="conv_bf16v3", form="conv", H=5, W=7, Cin=40, Cout=136, ncols_pad=192),    # three blocks, 8 channels in the last
    "v3_c192": dict(kernel="conv_bf16v3", form="conv", H=5, W=7, Cin=40, Cout=192, ncols_pad=192),    # second output: blocks 1 and 2
    "v3_c512": dict(kernel="conv_bf16v3", form="conv", H=5, W=7, Cin=40, Cout=512, ncols_pad=512),    # channel-block-major order
    # the ingest kernel over 9 x 40 cubes: two 32-wide tiles and one 8-wide one, so a workgroup's items change tile width
    "ig_c64": dict(kernel="conv_ingest", form="ingest", H=9, W=40, Cin=40, Cout=64, ncols_pad=128),   # second block: all masked
    "ig_c128": dict(kernel="conv_ingest", form="ingest", H=9, W=40, Cin=40, Cout=128, ncols_pad=128),
    "ig_c136": dict(kernel="conv_ingest", form="ingest", H=9, W=40, Cin=40, Cout=136, ncols_pad=192),
}
# With two blocks and an even nloc a workgroup's items k, k + nloc, ... all have the SAME block (item parity), so the bias slot of
# the previous item would do for the next one: the geometries with three blocks are the ones whose lists change block from item to
# item (``Mirror.block_changes``; nloc = CUs / 4 is 1 or 2 mod 3 at 256, 304 and 128 CUs).  In the channel-block-major order a band
# owns one block in eight, so with Cout_pad = 512 a workgroup keeps its block by design.
BLOCKS_CHANGE = ("f2_rows5_b3", "f2_convt", "g3_rows5_b3", "g3_convt", "v3_c136", "v3_c192", "ig_c136")


def geom_tiles(g):
    if g["form"] == "rows":
        return gemm_tiles(g["HW"])
    if g["form"] == "convt":
        return gemm_tiles(g["H"] * g["W"])
    if g["form"] == "conv":
        return v3_segments(g["H"], g["W"])[1]
    return ingest_segments(g["H"], g["W"])[1]


def geom_segments(g):
    """Column bands of one image for the kernels with 2-D tiles, None for the row kernels."""
    if g["form"] == "conv":
        return v3_segments(g["H"], g["W"])[0]
    if g["form"] == "ingest":
        return ingest_segments(g["H"], g["W"])[0]
    return None


def dgrad_ncols_pad(g):
    """The transposed convolution's data gradient has Cin output columns."""
    return rup(g["Cin"], 64)


@functools.lru_cache(maxsize=None)
def choose_images(geom, regime, ncu, ncols_pad=None):
    """The smallest image count, from a quarter into the regime on, whose work list meets every predicate of the regime (the
    predicates are checked on the mirror, not assumed)."""
    g = GEOMS[geom]
    t = geom_tiles(g)
    ncp = ncols_pad or g["ncols_pad"]
    lo, S = (2 if regime == "three_or_two" else 1), 2 * ncu
    per_image = t * cdiv(ncp, BLOCK[g["kernel"]])
    for N in range(cdiv(lo * S + S // 4, per_image), 4 * ncu):        # from a quarter into the regime: a quarter of the lists is long
        m = Mirror(g["kernel"], ncu, N * t, ncp)
        if m.items >= (lo + 1) * S:
            break
        if m.regime_holds(regime)[0]:
            return N
    raise AssertionError("no image count puts %s into %s at %d CUs" % (geom, regime, ncu))


def case_mirror(geom, regime, ncu, ncols_pad=None):
    g = GEOMS[geom]
    N = choose_images(geom, regime, ncu, ncols_pad)
    return N, Mirror(g["kernel"], ncu, N * geom_tiles(g), ncols_pad or g["ncols_pad"])


# ---------------------------------------------------------------------------------------------------------------------------
# Inputs (CPU, seeded, distinct per image because every image draws its own values) and fp64 references, cached per case
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(map(str, key)))))
    return g


SMALL, PRIOR = (-3, 3), (-8, 8)


@functools.lru_cache(maxsize=None)
def rows_case(geom, N):
    """Row GEMM y = x w^T + b: x [N*HW, K], w [C, K], bias [C], y0 [N*HW, C]; ref, budget."""
    g = GEOMS[geom]
    gen = _gen("rows", geom, N)
    P_ = N * g["HW"]
    x, w = _ints(gen, (P_, g["K"]), SMALL), _ints(gen, (g["C"], g["K"]), SMALL)
    bias, y0 = _ints(gen, (g["C"],), PRIOR), _ints(gen, (P_, g["C"]), PRIOR)
    ref = x.double() @ w.double().t()
    budget = float((x.double().abs() @ w.double().abs().t() + bias.double().abs() + y0.double().abs()).max())
    return dict(x=x, w=w, bias=bias, y0=y0, ref=ref, budget=budget)


@functools.lru_cache(maxsize=None)
def convt_case(geom, N):
    """ConvTranspose2d(k=2, s=2): x [N,H,W,Cin], wt [Cin,Cup,2,2], bias [Cup]; fwd [N,2H,2W,Cup] (without bias); dy [N,2H,2W,Cup]
    (the patch grid; the canvas around it is the test's), dx0 [N*H*W, Cin]; dgrad [N*H*W, Cin] = the adjoint of dy."""
    g = GEOMS[geom]
    gen = _gen("convt", geom, N)
    H, W, Cin, Cup = g["H"], g["W"], g["Cin"], g["Cup"]
    x, wt = _ints(gen, (N, H, W, Cin), SMALL), _ints(gen, (Cin, Cup, 2, 2), SMALL)
    bias, dy = _ints(gen, (Cup,), PRIOR), _ints(gen, (N, 2 * H, 2 * W, Cup), SMALL)
    dx0 = _ints(gen, (N * H * W, Cin), PRIOR)
    F = torch.nn.functional
    nchw = lambda t: t.double().permute(0, 3, 1, 2)
    fwd = F.conv_transpose2d(nchw(x), wt.double(), None, stride=2).permute(0, 2, 3, 1).contiguous()
    dgrad = F.conv2d(nchw(dy), wt.double(), stride=2).permute(0, 2, 3, 1).reshape(-1, Cin)
    b_fwd = float(F.conv_transpose2d(nchw(x.abs()), wt.double().abs(), bias.double().abs(), stride=2).max())
    b_dg = float((F.conv2d(nchw(dy.abs()), wt.double().abs(), stride=2).permute(0, 2, 3, 1).reshape(-1, Cin) + dx0.double().abs()).max())
    return dict(x=x, wt=wt, bias=bias, dy=dy, dx0=dx0, fwd=fwd, dgrad=dgrad, budget=max(b_fwd, b_dg))


@functools.lru_cache(maxsize=None)
def conv_case(geom, N):
    """3x3 pad-1 convolution: x [N,H,W,Cin], w [Cout,Cin,3,3] (the effective forward weight), bias [Cout], y0 [N*H*W, Cout];
    ref [N*H*W, Cout] without bias."""
    g = GEOMS[geom]
    gen = _gen("conv", geom, N)
    H, W, Cin, Cout = g["H"], g["W"], g["Cin"], g["Cout"]
    x, w = _ints(gen, (N, H, W, Cin), SMALL), _ints(gen, (Cout, Cin, 3, 3), SMALL)
    bias, y0 = _ints(gen, (Cout,), PRIOR), _ints(gen, (N * H * W, Cout), PRIOR)
    F = torch.nn.functional
    nchw = lambda t: t.double().permute(0, 3, 1, 2)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Cout)
    ref = rows(F.conv2d(nchw(x), w.double(), None, padding=1))
    budget = float((rows(F.conv2d(nchw(x.abs()), w.double().abs(), bias.double().abs(), padding=1)) + y0.double().abs()).max())
    return dict(x=x, w=w, bias=bias, y0=y0, ref=ref, budget=budget)


def round16(t, dtype):
    """The exact (fp64 integer) result rounded once to the 16-bit type, as its bits."""
    return t.to(dtype).view(torch.int16)


def tile_rows(g, N):
    """For every tile of the launch the rows (pixel indices of the [N*H*W, C] output) it owns: a list of index tensors."""
    if g["form"] in ("rows", "convt"):
        HW = g["HW"] if g["form"] == "rows" else g["H"] * g["W"]
        return [torch.arange(n * HW + p0, n * HW + min(HW, p0 + 256)) for n in range(N) for p0 in range(0, HW, 256)]
    segs, tiles = geom_segments(g), geom_tiles(g)
    H, W = g["H"], g["W"]
    tin = torch.tensor([[tile_in_image(segs, y, x) for x in range(W)] for y in range(H)]).reshape(-1)
    per = [torch.nonzero(tin == t).reshape(-1) for t in range(tiles)]
    return [n * H * W + per[t] for n in range(N) for t in range(tiles)]


def _tile_of_row(g, row):
    """(image, tile within the image) of output row ``row``."""
    if g["form"] in ("rows", "convt"):
        img, p = divmod(row, g["HW"] if g["form"] == "rows" else g["H"] * g["W"])
        return img, p // 256
    img, p = divmod(row, g["H"] * g["W"])
    return img, tile_in_image(geom_segments(g), p // g["W"], p % g["W"])


def first_wrong(g, N, mirror, bad, what=""):
    """``bad``: boolean [rows, columns] of wrong output elements (rows = pixels of the plain / low-resolution grid, columns = the
    launch's GEMM columns).  Names the first wrong item -- image, tile, block, and the workgroup and list position the mirror gives
    it -- and counts the wrong elements per list position: which step of the item loop broke."""
    idx = torch.nonzero(bad)
    if idx.numel() == 0:
        return ""
    tiles, bn = geom_tiles(g), BLOCK[mirror.kernel]
    row, col = int(idx[0, 0]), int(idx[0, 1])
    img, tin = _tile_of_row(g, row)
    per_pos = {}
    for r, c in {(r, c // bn) for r, c in idx.tolist()}:
        i, t = _tile_of_row(g, r)
        pos = mirror.owner[(i * tiles + t, c)][2]
        per_pos[pos] = per_pos.get(pos, 0) + 1
    return ("%s: %d wrong elements, first at row %d column %d = image %d, tile %d of it, block %d: %s; wrong (row, block) pairs per "
            "list position: %s") % (what, idx.shape[0], row, col, img, tin, col // bn, mirror.where(img * tiles + tin, col // bn),
                                   dict(sorted(per_pos.items())))


# ---------------------------------------------------------------------------------------------------------------------------
# A caller-owned item queue (GPU)
# ---------------------------------------------------------------------------------------------------------------------------
class _Queue:
    """A caller-owned queue on a stream of its own (so that nothing else in the test process shares its registration)."""

    def __init__(self, lib, dev="cuda:0"):
        self.lib = lib
        self.stream = torch.cuda.Stream(device=dev)
        self.h = ctypes.c_void_p(self.stream.cuda_stream)
        self.buf = torch.zeros(lib.hpri_item_queue_bytes() // 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def on(self):
        assert self.lib.hpri_set_item_queue(ctypes.c_void_p(self.buf.data_ptr()), self.buf.numel() * 4, self.h) == 0, self.lib.hpri_last_error()
        self.launches = 0                   # (registration resets the parity: the first launch draws from half 0)

    def next_half_is_zero(self, taken=True):
        """After a launch: the half the NEXT launch will draw from has been zeroed, the one just used holds its tickets.
        ``taken=False``: a launch whose workgroups have one item each keeps its fixed lists and leaves the queue alone."""
        if not taken:
            return int(self.buf.abs().sum()) == 0
        self.launches += 1
        h = self.buf.numel() // 2
        nxt = self.buf[:h] if self.launches % 2 == 0 else self.buf[h:]
        used = self.buf[h:] if self.launches % 2 == 0 else self.buf[:h]
        return int(nxt.abs().sum()) == 0 and int(used.abs().sum()) > 0

    def off(self):
        assert self.lib.hpri_set_item_queue(ctypes.c_void_p(0), 0, self.h) == 0
