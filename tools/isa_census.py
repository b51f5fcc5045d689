#!/usr/bin/env python3
"""Static instruction census of a kernel of the HIP library (VERDICT r4 item 5 ii: where do the ~1.0 non-MFMA vector instructions per
MFMA of conv_bf16v3 come from?): the kernel's gfx950 assembly (hipcc -S) split at its first and last v_mfma -- "before" (set-up),
"loop" (the k loop: everything between the first and the last MFMA) and "after" (epilogue + next item's set-up) -- with each
region's instructions by class.  A static count weights every instruction once; the k loop's body runs Cin_pad / 64 times per item
and the rest once, which the "per_item" estimate applies.   usage: isa_census.py conv_bf16v3.hip conv_bf16v3_kernel [chunks_per_item]

Second form, for a kernel with several k loops (conv_wino_wgrad_kernel: one per wave variant):
    isa_census.py --loops conv_wino.hip conv_wino_wgrad_kernel [mfmas_per_k_step] [--source FILE]
lists every innermost single-block loop that holds an MFMA, in the order of the listing: MFMAs, vector instructions by mnemonic,
LDS instructions by mnemonic, waits, per k-step (the loop's MFMAs / mfmas_per_k_step, default 8), what the loop around it holds
outside the k loop (the per-unit bookkeeping, counted statically), per unit loop what lies between its s_barrier and the first MFMA
behind it (scalar, vector, vector-memory, and the compares / selects / lane moves / multiplies among them), and the kernel's registers and scratch.  --source compiles another copy of the file (the parent's, say) with csrc/ as the include directory.

Third form, conv_wino4_kernel (its stage loop spans several basic blocks):
    isa_census.py --wino4 [--source FILE]
gives the stage loop per 32 MFMAs and the epilogue by phase (wino4_census)."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loops_census(argv):
    """Every innermost MFMA loop of one kernel: a label, no other label, and a conditional branch back to it."""
    source = None
    if "--source" in argv:
        i = argv.index("--source")
        source = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    src, kern = argv[0], argv[1]
    per_step = int(argv[2]) if len(argv) > 2 else 8
    csrc = os.path.join(ROOT, "hyperpri_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-S", "--cuda-device-only",
                               "-I", csrc, source or os.path.join(csrc, src), "-o", out], stderr=subprocess.DEVNULL)
        text = open(out).read()
    m = re.search(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\.Lfunc_end" % re.escape(kern), text, re.S | re.M)     # (the whole function: it may end in several places)
    name, body = m.group(1), m.group(2)

    def meta(key):
        mm = re.search(r"\.set %s\.%s, (\d+)" % (re.escape(name), key), text)
        return int(mm.group(1)) if mm else None

    # hipcc marks every block of a loop in the comment of its label ("in Loop: Header=BB0_43 Depth=1"; the inner loop's own
    # header: "Parent Loop BB0_43 Depth=1"): `outer` collects what a depth-1 loop holds outside its inner loops, i.e. the
    # per-unit bookkeeping around a k loop
    loops, label, block, where, outer, parent = [], None, [], None, {}, {}
    for ln in body.splitlines():
        lab = re.match(r"^(\.LBB\d+_\d+):(.*)", ln) or re.match(r"^; (%bb\.\d+):(.*)", ln)
        if lab:
            if lab.group(1).startswith("."):
                label, block = lab.group(1), []
            note = lab.group(2)
            hdr = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=1", note)
            par = re.search(r"Parent Loop (BB\d+_\d+) Depth=1", note)
            if "This Loop Header: Depth=1" in note:
                where = lab.group(1)[2:]
            elif hdr:
                where = hdr.group(1)
            elif par:
                where, parent[lab.group(1)] = None, par.group(1)
            else:
                where = None
            continue
        if not ln.startswith("\t") or ln.strip().startswith((";", ".")):
            continue
        tok = ln.split(";")[0].split()
        block.append(tok[0])
        if where:
            outer.setdefault(where, []).append(tok[0])
        if tok[0].startswith("s_cbranch") and tok[1] == label and any(x.startswith("v_mfma") for x in block):
            loops.append((label, block))

    def by_mnemonic(xs):
        c = {}
        for x in xs:
            x = re.sub(r"_e32$|_e64$", "", x)
            c[x] = c.get(x, 0) + 1
        return dict(sorted(c.items()))

    def barrier_to_first_mfma(header):
        """What a wave runs between the s_barrier at the top of the unit loop `header` and the first MFMA behind it: the blocks
        reachable from the barrier (branch targets and fall-through), each up to its first MFMA, every instruction counted once
        (static: both sides of every branch, so also the k-step's own operand reads and transform on the path it lies on)."""
        blocks, order, cur = {}, [], None
        for ln in body.splitlines():
            lab = re.match(r"^\.L(BB\d+_\d+):(.*)", ln) or re.match(r"^; (%bb\.\d+):(.*)", ln)
            if lab:
                cur = lab.group(1)
                order.append(cur)
                if cur == header or re.search(r"(Header=|Parent Loop )%s " % header, lab.group(2)):
                    blocks[cur] = []             # a block of this unit loop; the walk does not leave it
            elif cur in blocks and ln.startswith("\t") and not ln.strip().startswith((";", ".")):
                tok = ln.split(";")[0].split()
                blocks[cur].append((tok[0], tok[-1][2:] if tok[0].startswith(("s_cbranch", "s_branch")) else None))
        start = next((b for b in order if any(i == "s_barrier" for i, _ in blocks.get(b, []))), None)
        if start is None:
            return None
        seen, todo, got = set(), [(start, True)], []
        while todo:
            b, first = todo.pop()
            if b in seen and not first:
                continue
            seen.add(b)
            if b not in blocks:              # the loop's exit
                continue
            ins = blocks[b]
            if first:
                ins = ins[[i for i, _ in ins].index("s_barrier") + 1:]
            done = False
            for i, tgt in ins:
                if i.startswith("v_mfma"):
                    done = True
                    break
                got.append(i)
                if tgt and tgt not in seen:
                    todo.append((tgt, False))
                if i == "s_branch":
                    done = True
                    break
            if not done:
                nxt = order.index(b) + 1
                if nxt < len(order) and order[nxt] not in seen:
                    todo.append((order[nxt], False))
        valu = [x for x in got if x.startswith("v_")]
        bad = [x for x in got if x.startswith(("v_cmp", "v_cndmask", "v_readlane", "v_writelane", "v_readfirstlane", "s_mul_hi", "s_mul_i32"))]
        return {"scalar": sum(x.startswith("s_") and not x.startswith(("s_waitcnt", "s_nop")) for x in got), "vector": len(valu),
                "vector_memory": sum(x.startswith(("buffer_", "global_")) for x in got), "lds": sum(x.startswith("ds_") for x in got),
                "s_nop": sum(x == "s_nop" for x in got), "branches": sum(x.startswith(("s_cbranch", "s_branch")) for x in got),
                "vector_by_mnemonic": by_mnemonic(valu), "compares_selects_lane_moves_multiplies": by_mnemonic(bad)}

    rows = []
    for label, block in loops:
        mfma = sum(x.startswith("v_mfma") for x in block)
        steps = mfma / per_step
        valu = [x for x in block if x.startswith("v_") and not x.startswith("v_mfma")]
        lds = [x for x in block if x.startswith("ds_")]
        rows.append({"loop": label, "mfma": mfma, "k_steps_per_trip": steps,
                     "vector_per_k_step": round(len(valu) / steps, 2), "lds_per_k_step": round(len(lds) / steps, 2),
                     "vector": by_mnemonic(valu), "lds": by_mnemonic(lds),
                     "s_nop": sum(x == "s_nop" for x in block), "s_waitcnt": sum(x == "s_waitcnt" for x in block),
                     "packed_f32": sum(bool(re.match(r"v_pk_\w+_f32", x)) for x in block)})
        unit = outer.get(parent.get(label), [])
        rows[-1]["per_unit_outside_the_k_loop (static: both sides of every branch)"] = {
            "vector": sum(x.startswith("v_") for x in unit), "scalar": sum(x.startswith("s_") and not x.startswith(("s_waitcnt", "s_nop")) for x in unit),
            "vector_memory": sum(x.startswith(("buffer_", "global_")) for x in unit)}
    # per wave variant (= per depth-1 loop with a barrier, in the order of the listing): the unit boundary
    units = []
    for hdr in re.findall(r"^\.L(BB\d+_\d+):[^\n]*This Loop Header: Depth=1", body, re.M):
        c = barrier_to_first_mfma(hdr)
        if c:
            units.append({"unit_loop": hdr, "between_the_barrier_and_the_first_mfma": c})
    print(json.dumps({"kernel": name, "source": source or src, "vgprs": meta("num_vgpr"), "agprs": meta("num_agpr"),
                      "scratch_bytes": meta("private_seg_size"), "mfma_loops": rows, "unit_loops": units}, indent=1))


def wino4_census(argv):
    """conv_wino4_kernel: its stage loop spans several basic blocks (wave-uniform branches around the DMA issue), so --loops does
    not see it.  Stage loop: the blocks hipcc marks as part of a loop that holds MFMAs, per 32 MFMAs (one stage of one wave).  Epilogue: the
    diagnostics build (-DHPRI_STAMPS) carries an s_memtime at every STAMP; behind the last MFMA they come in source order -- 1, 4,
    then 5, 2, 3 once per epilogue variant -- and cut the listing into exchange | row transform + store | statistics + partial
    sums.  A static count: both sides of every branch inside a phase are counted once."""
    source = None
    if "--source" in argv:
        i = argv.index("--source")
        source = argv[i + 1]
    csrc = os.path.join(ROOT, "hyperpri_amd", "csrc")
    kern = "conv_wino4_kernel"

    def listing(extra):
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k.s")
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-S", "--cuda-device-only",
                                   *extra, "-I", csrc, source or os.path.join(csrc, "conv_wino4.hip"), "-o", out], stderr=subprocess.DEVNULL)
            text = open(out).read()
        m = re.search(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\.Lfunc_end" % kern, text, re.S | re.M)
        name, body = m.group(1), m.group(2)
        ins = [ln.split(";")[0].split()[0] for ln in body.splitlines() if ln.startswith("\t") and not ln.strip().startswith((";", "."))]
        meta = {k: int(re.search(r"\.set %s\.%s, (\d+)" % (re.escape(name), k), text).group(1)) for k in ("num_vgpr", "private_seg_size")}
        meta["lds_bytes"] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", text).group(1))
        return name, ins, meta, body

    def count(xs):
        valu = [re.sub(r"_e32$|_e64$", "", x) for x in xs if x.startswith("v_") and not x.startswith("v_mfma")]
        by = {}
        for x in valu:
            by[x] = by.get(x, 0) + 1
        return {"vector": len(valu), "lds": sum(x.startswith("ds_") for x in xs),
                "memory": sum(x.startswith(("buffer_", "global_", "flat_")) for x in xs), "barriers": sum(x == "s_barrier" for x in xs),
                "mfma": sum(x.startswith("v_mfma") for x in xs), "vector_by_mnemonic": dict(sorted(by.items()))}

    name, ins, meta, body = listing([])
    # blocks by the loop that holds them: hipcc names it in the comment of every block label
    groups, cur = {}, None
    for ln in body.splitlines():
        lab = re.match(r"^(\.LBB\d+_\d+):(.*)", ln) or re.match(r"^; (%bb\.\d+):(.*)", ln)
        if lab:
            note = lab.group(2)
            hdr = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d)", note)
            own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d)", note)
            cur = (hdr.group(1), int(hdr.group(2))) if hdr else (lab.group(1)[2:], int(own.group(1))) if own else None
            continue
        if cur and ln.startswith("\t") and not ln.strip().startswith((";", ".")):
            groups.setdefault(cur, []).append(ln.split(";")[0].split()[0])
    loops = {}
    for (hdr, depth), xs in groups.items():
        c = count(xs)
        if c["mfma"]:
            what = "steady stages (inner loop %s)" % hdr if depth == 2 else "first stage of a chunk and the halo DMA issue (chunk loop %s outside its inner loop)" % hdr
            loops[what] = {"stages_in_the_listing": c["mfma"] / 32.0, "vector_per_stage": round(c["vector"] / (c["mfma"] / 32.0), 2),
                           "lds_per_stage": round(c["lds"] / (c["mfma"] / 32.0), 2), **c}
    last = len(ins) - 1 - next(i for i, x in enumerate(reversed(ins)) if x.startswith("v_mfma"))
    whole = count(ins[last + 1:])
    _, dins, _, _ = listing(["-DHPRI_STAMPS"])
    dlast = len(dins) - 1 - next(i for i, x in enumerate(reversed(dins)) if x.startswith("v_mfma"))
    cuts = [i for i in range(dlast + 1, len(dins)) if dins[i] == "s_memtime"]
    assert len(cuts) >= 5 and (len(cuts) - 2) % 3 == 0, f"{len(cuts)} stamps behind the last MFMA"
    phases = {"exchange (column transform, plane writes)": count(dins[cuts[0]:cuts[1]])}
    for v in range((len(cuts) - 2) // 3):
        c5, c2, c3 = cuts[2 + 3 * v: 5 + 3 * v]
        store = count(dins[c5:c2])
        tag = "fast" if "buffer_store_dwordx4" in dins[c5:c2] else "general"
        phases[f"{tag}: row transform, bias, store (and the accumulate preload)"] = store
        phases[f"{tag}: statistics and BatchNorm-backward partial sums"] = count(dins[c2:c3])
    print(json.dumps({"kernel": name, "source": source or "conv_wino4.hip", "vgprs": meta["num_vgpr"], "scratch_bytes": meta["private_seg_size"],
                      "lds_bytes": meta["lds_bytes"],
                      "stage_loop (product build, static: both sides of every branch)": loops,
                      "behind_the_last_mfma (product build, both epilogue variants together)": whole,
                      "epilogue_by_phase (diagnostics build, cut at its stamps)": phases}, indent=1))


if len(sys.argv) > 1 and sys.argv[1] == "--wino4":
    wino4_census(sys.argv[2:])
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "--loops":
    loops_census(sys.argv[2:])
    sys.exit(0)
src, kern = sys.argv[1], sys.argv[2]
chunks = int(sys.argv[3]) if len(sys.argv) > 3 else 8
csrc = os.path.join(ROOT, "hyperpri_amd", "csrc")
with tempfile.TemporaryDirectory() as td:
    out = os.path.join(td, "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-S", "--cuda-device-only", "-I", csrc,
                           os.path.join(csrc, src), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
# the kernel's body: from its label to its s_endpgm
m = re.search(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(kern), text, re.S | re.M)
name, body = m.group(1), m.group(2)
ins = [ln.strip().split()[0] for ln in body.splitlines() if ln.startswith("\t") and not ln.strip().startswith((";", "."))]
first = next(i for i, x in enumerate(ins) if x.startswith("v_mfma"))
last = len(ins) - 1 - next(i for i, x in enumerate(reversed(ins)) if x.startswith("v_mfma"))


def klass(x):
    if x.startswith("v_mfma"):
        return "mfma"
    if x.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "valu_lane_moves (SGPR spills / uniform values)"
    if x.startswith("v_"):
        return "valu_other"
    if x.startswith("ds_"):
        return "lds"
    if x.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if x.startswith(("s_waitcnt", "s_barrier", "s_nop", "s_sleep", "s_setprio")):
        return "sync"
    if x.startswith("s_"):
        return "salu"
    return "other"


def census(lo, hi):
    c = {}
    for x in ins[lo:hi]:
        c[klass(x)] = c.get(klass(x), 0) + 1
    return c


regions = {"before_first_mfma": census(0, first), "k_loop (first to last mfma, both copies of the unrolled body)": census(first, last + 1),
           "after_last_mfma": census(last + 1, len(ins))}
loop = regions["k_loop (first to last mfma, both copies of the unrolled body)"]
# the unrolled body holds two chunks: it runs chunks / 2 times per item
times = chunks / 2.0
per_item = {"mfma": loop.get("mfma", 0) * times}
for k in ("valu_other", "valu_lane_moves (SGPR spills / uniform values)"):
    per_item[k + " in the k loop"] = loop.get(k, 0) * times
    per_item[k + " outside"] = regions["before_first_mfma"].get(k, 0) * 0 + regions["after_last_mfma"].get(k, 0)
valu_in = per_item["valu_other in the k loop"] + per_item["valu_lane_moves (SGPR spills / uniform values) in the k loop"]
valu_out = per_item["valu_other outside"] + per_item["valu_lane_moves (SGPR spills / uniform values) outside"]
print(json.dumps({"kernel": name, "source": src, "static_instruction_counts": regions, "chunks_per_item": chunks,
                  "per_item_estimate": per_item, "non_mfma_valu_per_mfma": {"k_loop": round(valu_in / per_item["mfma"], 3),
                                                                            "epilogue_and_setup": round(valu_out / per_item["mfma"], 3)}}, indent=1))
