#!/usr/bin/env python3
"""The memory levels a wave of the packed sim3 kernels goes through in series, read from the listing of a part (the same
device-only compile as tools/hot_path_bytes.py, csrc/Makefile's flags for the family).
Per kernel of the part:
  entry   every memory instruction (scalar and global loads, LDS writes) and every wait, in layout order from the kernel's first instruction to
          the first LDS READ (the FK seed's), with the source line; a wait that has a load of its kind outstanding closes a LEVEL. Waits for
          kernel-argument words alone (scalar loads through the kernarg pointer s[0:1]) are counted apart: they hit the constant cache.
  late    every later global load of the hot path whose next vmcnt wait comes before `--near` (default 100) other instructions: a round trip
          waited for (almost) on the spot. The wave order's `cur` (wbc_packed.h wo_post) is expected here (§3.23).
Blocks reachable only through a `; WBC_COLD` / `; WBC_TAIL_BEGIN` marker are left out. Static evidence: the layout order is the order a wave
that takes every hot block walks through. CPU only:
    python tools/entry_levels.py [--near N] [--src DIR] [family.part ...]      (default sim3p.9; --src: another checkout's csrc; WBC_XFLAGS adds flags)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mech5845m-wbc-for-legged-manipulator_amd", "csrc")
NPARTS = {"sim3p": 12}


def listing(part, csrc):
    fam, k = part.split(".")
    flags = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", csrc, "family-flags", "FAM=" + fam], text=True).split()
    out = os.path.join(tempfile.gettempdir(), "wbc_levels_%s_%s_%d.s" % (fam, k, os.getpid()))
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S", "-g1",
                           "-D%s_PART=%s" % (fam.upper(), k), *flags, "-DWBC_NPARTS=%d" % NPARTS.get(fam, 1)] + os.environ.get("WBC_XFLAGS", "").split()
                          + [os.path.join(csrc, "wbc_k_%s.hip" % fam), "-o", out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    os.unlink(out)
    return txt


def hot_instructions(body, files):
    """-> [(instruction, source line)] of the blocks not reached through a cold marker alone, in layout order"""
    blocks, cur, where = [], {"label": "entry", "ins": [], "succ": [], "fall": True, "cut": False}, "?"
    for line in body.splitlines():
        loc = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", line)
        if loc:
            where = "%s:%s" % (files.get(loc.group(1), "file" + loc.group(1)), loc.group(2))
            continue
        if re.match(r"\s*\.section", line):
            break
        if re.match(r"\s*;\s*(WBC_COLD|WBC_TAIL_BEGIN)\s*$", line):
            cur["cut"] = True
            continue
        lab = re.match(r"^(\.LBB\w+):", line)
        if lab:
            blocks.append(cur)
            cur = {"label": lab.group(1), "ins": [], "succ": [], "fall": True, "cut": False}
            continue
        ins = line.split(";")[0].strip()
        if not ins or ins.startswith(".") or ins.endswith(":"):
            continue
        if cur["cut"]:
            continue
        cur["ins"].append((ins, where))
        br = re.match(r"s_(c?branch\w*)\s+(\.LBB\w+)", ins)
        if br:
            cur["succ"].append(br.group(2))
            if br.group(1) == "branch":
                cur["fall"] = False
        if ins.startswith("s_endpgm") or ins.startswith("s_setpc"):
            cur["fall"] = False
    blocks.append(cur)
    index = {b["label"]: i for i, b in enumerate(blocks)}
    seen, stack = set(), [0]
    while stack:
        i = stack.pop()
        if i in seen or i >= len(blocks):
            continue
        seen.add(i)
        stack.extend(index[t] for t in blocks[i]["succ"] if t in index)
        if blocks[i]["fall"] and not blocks[i]["cut"]:
            stack.append(i + 1)
    return [x for i in sorted(seen) for x in blocks[i]["ins"]]


def kind(ins):
    mn = ins.split()[0]
    if mn.startswith("s_load") or mn.startswith("s_buffer_load"):
        return "karg" if re.search(r",\s*s\[0:1\]", ins) else "smem"
    if re.match(r"(global|flat|buffer)_", mn):          # (stores count in vmcnt as well)
        return "vmem"
    if mn.startswith("scratch_load"):
        return "scratch"
    if mn.startswith("ds_read") or mn.startswith("ds_load") or mn.startswith("ds_bpermute") or mn.startswith("ds_permute"):
        return "ldsr"
    if mn.startswith("ds_"):
        return "ldsw"
    if mn.startswith("s_waitcnt"):
        return "wait"
    return None


def analyse(part, near, csrc):
    txt = listing(part, csrc)
    files = {m.group(1): os.path.basename(m.group(2)) for m in re.finditer(r'^\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', txt, re.M)}
    for m in re.finditer(r"^(_ZN3wbc\w+):[^\n]*\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
        name = subprocess.check_output(["c++filt", m.group(1)], text=True).strip()
        name = re.sub(r"\(.*", "", name.replace("void wbc::", ""))
        ins = hot_instructions(m.group(2), files)
        print("== %s  (%s)" % (name, part))
        print("-- entry: memory instructions and waits up to the first LDS read")
        pend = {"karg": 0, "smem": 0, "vmem": 0}
        levels = karg_levels = 0
        end = len(ins)
        for i, (x, where) in enumerate(ins):
            k = kind(x)
            if k is None or k == "scratch":
                continue
            if k == "ldsr":
                print("   %5d  %-58s %s   <- first LDS read" % (i, x, where))
                end = i
                break
            note = ""
            if k in pend:
                pend[k] += 1
            elif k == "wait":
                lg, vm = re.search(r"lgkmcnt\((\d+)\)", x), re.search(r"vmcnt\((\d+)\)", x)
                closed = []
                if vm and pend["vmem"] > int(vm.group(1)):
                    closed.append("%d global" % (pend["vmem"] - int(vm.group(1))))
                    pend["vmem"] = int(vm.group(1))
                if lg and pend["smem"] + pend["karg"] > int(lg.group(1)):
                    if pend["smem"]:
                        closed.append("%d scalar" % pend["smem"])
                    elif not closed:
                        closed.append("%d kernel-argument" % pend["karg"])
                    pend["smem"] = pend["karg"] = 0
                if closed and closed[0].endswith("kernel-argument"):
                    karg_levels += 1
                    note = "   == kernel-argument wait %d (%s)" % (karg_levels, closed[0])
                elif closed:
                    levels += 1
                    note = "   == LEVEL %d closes (%s)" % (levels, ", ".join(closed))
            print("   %5d  %-58s %s%s" % (i, x, where, note))
        print("-- entry: %d serial memory level(s) and %d kernel-argument wait(s) before the first LDS read" % (levels, karg_levels))
        print("-- late: global loads waited for within %d instructions" % near)
        n_late = 0
        for i in range(end, len(ins)):
            x, where = ins[i]
            if kind(x) != "vmem" or not re.match(r"(global|flat|buffer)_load", x):
                continue
            after = 0
            for j in range(i + 1, min(len(ins), i + 1 + near + 1)):
                y = ins[j][0]
                if y.startswith("s_waitcnt") and re.search(r"vmcnt\(", y):
                    later = sum(1 for t in range(i + 1, j) if kind(ins[t][0]) == "vmem")
                    if int(re.search(r"vmcnt\((\d+)\)", y).group(1)) <= later:
                        print("   %5d  %-58s %s   waited for after %d instruction(s)" % (i, x, where, after))
                        n_late += 1
                        break
                after += 1
        print("-- late: %d" % n_late)


def main():
    args = sys.argv[1:]
    near, csrc, parts = 100, CSRC, []
    while args:
        a = args.pop(0)
        if a == "--near":
            near = int(args.pop(0))
        elif a == "--src":
            csrc = os.path.abspath(args.pop(0))
        else:
            parts.append(a)
    for part in parts or ["sim3p.9"]:
        analyse(part, near, csrc)


if __name__ == "__main__":
    main()
