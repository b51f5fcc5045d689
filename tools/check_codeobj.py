#!/usr/bin/env python3
"""Register-spill gate for the hot-path kernels.

Compiles every csrc/*.hip DEVICE-ONLY for gfx950 with the product's flags plus ``-Rpass-analysis=kernel-resource-usage`` and
reads, per kernel, what the code object's metadata holds as ``.vgpr_count`` / ``.vgpr_spill_count`` / ``.sgpr_spill_count`` /
``.private_segment_fixed_size`` (the remarks print the same numbers: "VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize").
A kernel of the hot-path list with a spilled register or a non-zero scratch size fails the check (exit code 1), with ONE
tolerated class (TOLERATED below): kernels whose few spilled registers are written and re-read OUTSIDE the range of their
k loop -- the tool proves that from the ISA (no scratch_* instruction inside a loop that holds a v_mfma) and holds the scratch
size to the stated bound.

    python tools/check_codeobj.py            # table of every kernel + verdict
    python tools/check_codeobj.py --json     # the same as one JSON object (tests/test_codeobj.py reads this)

Each row also carries ``max_flat_wg``: the kernel's ``.max_flat_workgroup_size`` from the same metadata (its __launch_bounds__,
1024 without one) -- with ``vgprs`` and ``lds`` what decides whether a workgroup can be placed on a compute unit beside a resident
workgroup of another kernel (tests/test_codeobj_coresident.py).

No GPU needed (hipcc cross-compiles).  Results are cached on the source stamp under hyperpri_amd/lib/.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hyperpri_amd import build as B  # noqa: E402

# Kernels a training / predict step of the BASELINE configs launches (demangled-name prefixes): these must hold every value in
# registers.  Anything else in the library is reported, not gated.
HOT = (
    "conv_wino4_kernel", "conv_wino_wgrad_kernel", "wino_wgrad_reduce_kernel", "wino_wgrad_reduce_wide_kernel",
    "conv_bf16v3_kernel", "conv_wgrad_bf16v2_kernel", "gemm_bf16v3_kernel", "gemm_f32v2_kernel", "wgrad1x1_bf16v3_kernel",
    "conv_fwd_kernel", "conv_wgrad_kernel", "splitk_finish_kernel", "wgrad_reduce", "conv_wino6", "wino6",
    "bn_", "col_", "maxpool2", "nchw_to_nhwc", "outconv", "bce_", "adam", "copy_slice", "fill_pad", "to_planes",
    "cube_gather_kernel", "mask_gather_kernel", "cube_warp_kernel", "mask_warp_kernel", "cube_deform_kernel", "mask_deform_kernel", "elastic_field_kernel", "seg_loss_", "tta_merge_",
    "band_moments_kernel", "band_gram_kernel", "band_project_kernel", "band_affine_kernel", "band_assign_kernel", "band_cluster_kernel", "band_gmm_score_kernel", "band_gmm_sums_kernel",
    "band_unmix_kernel", "band_extreme_kernel", "guided_coeff_kernel", "guided_apply_kernel", "ridge_filter_kernel", "crf_iter_kernel", "crf_back_kernel",
    "soft_skel_fwd_kernel", "soft_skel_bwd_kernel", "cldice_finalize_kernel", "centerline_count_kernel",
    "sort_hist_kernel", "sort_count_kernel", "sort_scan_kernel", "sort_scatter_kernel", "sort_finish_kernel", "lz_", "rk_",
)

# conv_fwd_kernel<KS, 2, 2, ...> (fp32 direct kernel at three workgroups per CU = 168 registers; it needs 170 for a few
# instructions of its epilogue's bias pass -- five source-level reformulations of that pass, 32-bit store offsets and
# scheduling fences left the count where it was): 2 registers, stored and reloaded once each, after the k loop.
TOLERATED = {"conv_fwd_kernel": 16}          # name prefix -> largest scratch size in bytes per lane


def _scratch_outside_mfma(src, mangled):
    """True when no scratch_* instruction of kernel ``mangled`` lies inside a loop of its ISA that holds a v_mfma."""
    cmd = [B._hipcc(), *B.FLAGS, "-x", "hip", "--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-I", B.CSRC, "-o", "-"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    if r.returncode != 0:
        return False
    lines = r.stdout.splitlines()
    start = next((i for i, ln in enumerate(lines) if ln.startswith(mangled + ":")), None)
    if start is None:
        return False
    body = []
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):          # (an early return leaves s_endpgm inside the body)
            break
        body.append(ln)
    # loops = backward branches: [line of the target label, line of the branch]; a scratch access is "in the k loop" when it
    # lies inside a loop that also holds a matrix instruction
    labels = {ln.split(":")[0]: i for i, ln in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", ln)}
    loops = []
    for i, ln in enumerate(body):
        m = re.search(r"\bs_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            t = labels[m.group(1)]
            # (a branch back to a shared exit block -- label, a few instructions, s_endpgm -- is no loop)
            nxt = next((ln2 for ln2 in body[t + 1:] if re.match(r"^\.LBB", ln2) or "s_endpgm" in ln2 or re.search(r"\bs_c?branch", ln2)), "")
            if "s_endpgm" not in nxt:
                loops.append((t, i))
    mf = [i for i, ln in enumerate(body) if "v_mfma" in ln]
    sc = [i for i, ln in enumerate(body) if "scratch_" in ln]
    hot_loops = [(a, b) for a, b in loops if any(a <= j <= b for j in mf)]
    return bool(mf) and not any(a <= i <= b for i in sc for a, b in hot_loops)


_FIELDS = {"Function Name": "name", "TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
           "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill",
           "LDS Size [bytes/block]": "lds"}


def _demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return out.stdout.split("\n")[:len(names)]
    except Exception:
        return names


def _readelf():
    hipcc = shutil.which(B._hipcc()) or B._hipcc()
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "llvm-readelf"), os.path.join(rocm, "llvm", "bin", "llvm-readelf"),
              "/opt/rocm/lib/llvm/bin/llvm-readelf", shutil.which("llvm-readelf")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("llvm-readelf not found")


def _max_flat_workgroup_sizes(codeobj):
    """{mangled kernel name: .max_flat_workgroup_size} from the metadata note of a device code object."""
    r = subprocess.run([_readelf(), "--notes", codeobj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"llvm-readelf failed on {codeobj}:\n{r.stdout[-2000:]}")
    out, size = {}, None
    for line in r.stdout.splitlines():          # a kernel's own keys sit at four spaces (its arguments' deeper), sorted by name
        m = re.match(r"^    \.max_flat_workgroup_size:\s+(\d+)", line)
        if m:
            size = int(m.group(1))
            continue
        m = re.match(r"^    \.name:\s+(\S+)", line)
        if m and size is not None:
            out[m.group(1)] = size
            size = None
    return out


def analyse(src):
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, src.rsplit(".", 1)[0] + ".co")
        cmd = [B._hipcc(), *B.FLAGS, "-x", "hip", "--cuda-device-only", "--no-gpu-bundle-output", "-c", os.path.join(B.CSRC, src),
               "-I", B.CSRC, "-Rpass-analysis=kernel-resource-usage", "-o", co]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout[-4000:]}")
        flat = _max_flat_workgroup_sizes(co)
    kernels, cur = [], None
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"file": src, "name": val}
            kernels.append(cur)
        elif cur is not None and key in _FIELDS:
            cur[_FIELDS[key]] = int(val)
    for k, d in zip(kernels, _demangle([k["name"] for k in kernels])):
        k["demangled"] = d
        if k["name"] in flat:                    # (device functions that are no kernels have remarks but no metadata entry)
            k["max_flat_wg"] = flat[k["name"]]
    return kernels


def run(force=False):
    stamp = hashlib.sha256((B._stamp() + open(__file__).read()).encode()).hexdigest()
    cache = os.path.join(B.LIBDIR, "codeobj_report.json")
    if not force and os.path.exists(cache):
        try:
            got = json.load(open(cache))
            if got.get("stamp") == stamp:
                return got
        except Exception:
            pass
    srcs = [s for s in B.SOURCES if s.endswith(".hip")]
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        rows = [k for ks in ex.map(analyse, srcs) for k in ks]
    bad = []
    for k in rows:
        base = k["demangled"].split("(")[0].replace("void ", "")
        k["hot"] = any(base.startswith(h) for h in HOT)
        # (scalar registers parked in lanes of a vector register -- "SGPRs Spill" -- touch no memory: reported, not gated)
        k["clean"] = k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0
        k["tolerated"] = False
        if k["hot"] and not k["clean"]:
            lim = next((v for h, v in TOLERATED.items() if base.startswith(h)), None)
            if lim is not None and k.get("scratch", 0) <= lim and _scratch_outside_mfma(k["file"], k["name"]):
                k["tolerated"] = True
            else:
                bad.append(k["demangled"])
    out = {"stamp": stamp, "kernels": rows, "hot_path_kernels_with_spills": bad, "ok": not bad}
    os.makedirs(B.LIBDIR, exist_ok=True)
    with open(cache, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    return out


def main():
    rep = run(force="--force" in sys.argv)
    if "--json" in sys.argv:
        print(json.dumps(rep))
    else:
        for k in sorted(rep["kernels"], key=lambda k: (k["file"], k["demangled"])):
            flag = "" if k["clean"] else ("  <-- spill outside the k loop (tolerated)" if k.get("tolerated") else
                                          "  <-- SPILL (hot path)" if k["hot"] else "  <-- spill (not gated)")
            print(f"{k['file']:24s} {k['demangled'][:78]:78s} vgpr {k.get('vgprs', 0):3d} agpr {k.get('agprs', 0):3d} scratch {k.get('scratch', 0):4d} "
                  f"vspill {k.get('vgpr_spill', 0):3d} sspill {k.get('sgpr_spill', 0):3d} occ {k.get('occupancy', 0)}{flag}")
        print("OK: no hot-path kernel spills" if rep["ok"] else "FAIL: " + "; ".join(rep["hot_path_kernels_with_spills"]))
    return 0 if rep["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
