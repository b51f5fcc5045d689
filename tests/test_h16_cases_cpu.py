"""The premises of test_gpu_h16_kernels.py, proved without a device (_h16_cases.py): integer operands are exact in both 16-bit types
and their budgets stay below 2^24; real operands are exact in the library's type; every edge-table operand is a value of the type,
every edge-table output is lossless in fp32 and the expected bits hold every class the table is for; and the real-valued bound
(n + 2) u (sum |a||b| + |bias| + |prior|) is neither too tight nor vacuous: fp32 evaluations of the same sums in two orders stay
inside it, while a reference with the last k-step of 32 dropped, with the input shifted by one pixel or with two output channels
swapped exceeds it on at least one element -- for every real case of both libraries."""
import pytest
import torch

import _h16_cases as HC

KINDS = ("int", "real")


def _names(kind):
    return [name for name, _ in HC.bilinear_cases(kind, "bf16")]


def _case(kind, lib, name):
    return dict(HC.bilinear_cases(kind, lib))[name]


@pytest.mark.parametrize("lib", HC.LIBS)
def test_operands_are_exact_in_the_16_bit_type(lib):
    """Integer operands survive .to(dtype) in BOTH types (the integer cases of one library are also valid in the other), real ones
    in the type of their library."""
    for kind in KINDS:
        for name, c in HC.bilinear_cases(kind, lib):
            for dt in (HC.DTYPES.values() if kind == "int" else [HC.DTYPES[lib]]):
                for k in ("a", "b"):
                    assert torch.equal(c[k].to(dt).float(), c[k]), (name, kind, k, dt)
            assert c["ref"].dtype == torch.float64 and c["mag"].shape == c["ref"].shape and c["prior"].shape == c["ref"].shape
    for kind in KINDS:
        for s in HC.POOL:
            p = HC.pool_case(kind, lib, s)
            assert torch.equal(p["x"].to(HC.DTYPES[lib]).float(), p["x"])
            N, H, W, C = s
            win = p["x"][:, :H // 2 * 2, :W // 2 * 2].reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)
            ties = (win == win.max(-1, keepdim=True).values).sum(-1) > 1
            assert int(ties.sum()) > ties.numel() // 8, "the windows must hold ties at their maximum"
            assert int((p["routed"] != 0).sum()) <= p["dy"].numel() and torch.equal(p["routed"].reshape(N, H, W, C).sum((1, 2)), p["dy"].double().sum((1, 2)))


@pytest.mark.parametrize("lib", HC.LIBS)
def test_integer_budgets_are_below_2_to_the_24(lib):
    for name, c in HC.bilinear_cases("int", lib):
        assert HC.budget(c) < HC.LIMIT, (name, HC.budget(c))
        assert torch.equal(c["ref"], c["ref"].round()) and torch.equal(c["ref"].float().double(), c["ref"])
    for s in HC.HEAD:
        h = HC.head_case("int", lib, s)
        assert float(h["db_mag"].max()) + 8 < HC.LIMIT


@pytest.mark.parametrize("lib", HC.LIBS)
@pytest.mark.parametrize("form", sorted(HC.EDGE))
def test_edge_tables(lib, form):
    """Operands are values of the type (no inf, NaN or -0), outputs are lossless in fp32 and normal there, the selector has at most
    two non-zeros per column, each a power of two, and the expected bits hold one of each class the table is for."""
    rows, K, ncols, single = HC.EDGE[form]
    dt = HC.DTYPES[lib]
    e = HC.edge_problem(lib, rows, K, ncols, single)
    A, B, y64 = e["A"], e["B"], e["y64"]
    for t in (A, B):
        assert torch.isfinite(t).all() and torch.equal(t.to(dt).float(), t)
        assert not bool(((t == 0) & torch.signbit(t)).any())
    nz = (B != 0).sum(1)
    assert int(nz.max()) <= (1 if single else 2) and int(nz.min()) >= 1
    m, _ = torch.frexp(B[B != 0])
    assert bool((m == 0.5).all())                                          # powers of two
    assert torch.equal(y64, y64.float().double())                          # lossless in fp32
    assert float(y64.abs().min()) >= 2.0 ** -126                           # ... and a normal fp32
    want = y64.float().to(dt)
    assert torch.equal(HC.round16(y64.float(), dt), e["bits"]) and torch.equal(want.view(torch.int16), e["bits"])
    fi = torch.finfo(dt)
    cls = lambda name: e["cls"] == HC.CLASSES.index(name)
    exact = want.double() == y64
    assert bool(exact[cls("exact")].all()) and int(cls("exact").sum()) > 0
    intended = ["exact"] if single else ["exact", "tie rounded down", "tie rounded up"]
    if dt == torch.float16:
        intended += ["subnormal", "subnormal operand", "inf"] if not single else ["subnormal", "subnormal operand", "inf", "tie rounded down", "tie rounded up"]
    for name in intended:
        assert int(cls(name).sum()) > 0, name
    assert not bool(exact[cls("tie rounded down")].any()) and not bool(exact[cls("tie rounded up")].any())
    down, up = cls("tie rounded down"), cls("tie rounded up")
    assert bool((want.double().abs()[down] < y64.abs()[down]).all()) and bool((want.double().abs()[up] > y64.abs()[up]).all())
    if dt == torch.float16:
        assert bool(torch.isinf(want[cls("inf")]).all()) and int(torch.isinf(want).sum()) == int(cls("inf").sum())
        sub = (want != 0) & (want.abs().float() < fi.smallest_normal)
        assert bool(sub[cls("subnormal")].all())
        assert bool(((A != 0) & (A.abs() < fi.smallest_normal)).any())     # subnormal operands go in
        assert int((want == 0).sum()) > 0                                  # 2^-25 rounds to zero, never the other way round
    else:
        assert bool(torch.isfinite(want).all())


@pytest.mark.parametrize("lib", HC.LIBS)
@pytest.mark.parametrize("name", _names("real"))
def test_real_bound_is_not_vacuous(lib, name):
    """fp32 evaluations stay inside the bound; each mutation exceeds it somewhere."""
    c = _case("real", lib, name)
    b = HC.bound(c)
    assert float(b.min()) >= 0 and torch.isfinite(b).all()
    for how, got in HC.emulations(c).items():
        r = ((got - c["ref"]).abs() / b.clamp_min(1e-300)).max()
        assert float(r) <= 1.0, (name, how, float(r))
    for how, mut in HC.mutations(c).items():
        r = ((mut - c["ref"]).abs() / b.clamp_min(1e-300)).max()
        assert float(r) > 1.0, (name, how, float(r))
