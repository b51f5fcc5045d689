"""Co-residency budgets of the two streams of the fp32 backward, from the code-object report alone.

The backward runs the Winograd weight gradient on a side stream beside the main stream's BatchNorm-backward sweeps, and the
many-slab weight-gradient reduce on the side stream beside the main stream's data gradient.  A workgroup can only be placed on
a compute unit where its whole register and LDS demand is free, so a small kernel whose WORKGROUP is large waits for the long
kernel's workgroups to retire and the overlap is lost.  This checks, per SIMD and per compute unit:

    waves per SIMD x registers of a wave (allocated in blocks of 8)  <=  512 - what the resident workgroup(s) hold
    LDS of the workgroup                                              <=  160 KiB - what the resident workgroup(s) hold

Figures come from tools/check_codeobj.py (registers, LDS and the maximum flat workgroup size of every kernel); only the sizes
of the register file and of the LDS are constants here.  No GPU needed; no assembly is read."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

REGS_PER_SIMD = 512              # vector registers per lane of one SIMD (unified VGPR + AGPR file)
REG_BLOCK = 8                    # allocation granularity
LDS_PER_CU = 160 * 1024
SIMDS, WAVE = 4, 64


def _base(k):
    return k["demangled"].split("(")[0].replace("void ", "")


def _regs(k):
    r = k.get("vgprs", 0) + k.get("agprs", 0)
    return (r + REG_BLOCK - 1) // REG_BLOCK * REG_BLOCK


def _waves_per_simd(k):
    assert "max_flat_wg" in k, f"{_base(k)}: the report lacks the maximum flat workgroup size"
    waves = (k["max_flat_wg"] + WAVE - 1) // WAVE
    return (waves + SIMDS - 1) // SIMDS


def _one(rep, name):
    got = [k for k in rep["kernels"] if _base(k) == name]
    assert len(got) == 1, f"{name}: {len(got)} entries in the code-object report"
    return got[0]


def _fits_beside(k, resident, copies):
    """(registers needed per SIMD, registers free, LDS needed, LDS free) of workgroup `k` beside `copies` resident workgroups."""
    need = _waves_per_simd(k) * _regs(k)
    free = REGS_PER_SIMD - copies * _waves_per_simd(resident) * _regs(resident)
    return need, free, k.get("lds", 0), LDS_PER_CU - copies * resident.get("lds", 0)


def test_main_stream_sweeps_fit_beside_a_weight_gradient_workgroup():
    """col_fold / col_finalize and every col_reduce / bn_bwd_apply / bn_pool_bwd instantiation beside ONE resident
    conv_wino_wgrad_kernel workgroup (it runs one per compute unit and sits on all of them while it runs)."""
    import check_codeobj as C
    rep = C.run()
    wgrad = _one(rep, "conv_wino_wgrad_kernel")
    sweeps = [k for k in rep["kernels"]
              if _base(k).startswith(("col_fold_kernel", "col_finalize_kernel", "col_reduce_kernel", "bn_bwd_apply_kernel", "bn_pool_bwd_kernel"))]
    names = {_base(k) for k in sweeps}
    for must in ("col_fold_kernel<8>", "col_finalize_kernel<8>", "col_reduce_kernel<0, false, false>", "col_reduce_kernel<1, false, false>",
                 "bn_bwd_apply_kernel<false, false>", "bn_pool_bwd_kernel<false>", "bn_pool_bwd_kernel<true>"):
        assert must in names, f"{must} missing from the code-object report"
    for k in sweeps:
        need, free, lds, lds_free = _fits_beside(k, wgrad, 1)
        assert need <= free, f"{_base(k)}: {need} registers per SIMD, {free} free beside conv_wino_wgrad_kernel"
        assert lds <= lds_free, f"{_base(k)}: {lds} bytes of LDS, {lds_free} free beside conv_wino_wgrad_kernel"


def test_many_slab_reduce_fits_beside_one_data_gradient_workgroup():
    """wino_wgrad_reduce_wide_kernel<16> beside ONE resident conv_wino4_kernel workgroup (two run per compute unit: the reduce is
    placed as soon as either has left)."""
    import check_codeobj as C
    rep = C.run()
    wino4 = _one(rep, "conv_wino4_kernel")
    k = _one(rep, "wino_wgrad_reduce_wide_kernel<16>")
    need, free, lds, lds_free = _fits_beside(k, wino4, 1)
    assert need <= free, f"{need} registers per SIMD, {free} free beside one conv_wino4_kernel workgroup"
    assert lds <= lds_free, f"{lds} bytes of LDS, {lds_free} free beside one conv_wino4_kernel workgroup"
    # and the premise: two conv_wino4_kernel workgroups do fit a compute unit together
    assert 2 * _waves_per_simd(wino4) * _regs(wino4) <= REGS_PER_SIMD and 2 * wino4.get("lds", 0) <= LDS_PER_CU
