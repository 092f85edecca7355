#!/usr/bin/env python3
"""How large the instruction stream of the packed sim3 kernels' hot path is, and where the compiler put it.
Same device-only listing as tools/hot_path_spills.py (hipcc -S -g1), re-read through llvm-mc -show-encoding for the size of every instruction.
A block is COLD if it can be reached only through a `; WBC_COLD` comment (COLD_MARK() at the head of a rarely taken block of wbc_k_sim3p.hip) or
through `; WBC_TAIL_BEGIN` (the general-path tail); everything else reachable from the kernel's entry is HOT. Printed per kernel variant:
  hot      instructions and bytes of the hot blocks
  span     bytes from the kernel's entry to the end of the LAST hot block in layout order: the stream a wave walks through
  inside   bytes of cold blocks (and padding) that lie inside that span: what the wave's fetches pass over without running it
  rest     bytes of everything behind the span (cold blocks and the tail)
  hot scratch ld/st   scratch_load / scratch_store instructions in the hot blocks (tools/hot_path_spills.py counts the cold blocks in as well)
The layout without the hints and the family's flag (the parent's): WBC_XFLAGS=-DSIM3P_NO_LAYOUT_HINTS FAMFLAGS_sim3p= .
CPU only (cross-compiles):
    python tools/hot_path_bytes.py [-v] [--mix] [family.part ...]      -v: the layout as runs of hot / cold bytes; default: every sim3p part   (WBC_XFLAGS="-D..." adds compiler flags)
--mix: what the hot path is made of — its instructions by class (fp64 arithmetic; moves of an immediate and of a register;
selects; DPP; other VALU; scalar; exec-mask handling: saveexec, branches on exec, writes to exec; waits; nops; LDS; global and scratch) and,
per class, the source lines that own most of them (the -g1 line tables; an inlined helper's instructions count for the helper's own line)."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mech5845m-wbc-for-legged-manipulator_amd", "csrc")
NPARTS = {"sim3p": 12}


def llvm_mc():
    hipcc = subprocess.check_output(["which", "hipcc"], text=True).strip()
    for d in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin"), os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin"),
              "/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin"):
        p = os.path.join(d, "llvm-mc")
        if os.path.exists(p):
            return p
    return "llvm-mc"


def family_flags(fam):
    """the flags csrc/Makefile gives this family's parts alone (FAMFLAGS_<family>)"""
    return subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "family-flags", "FAM=" + fam], text=True).split()


def listing(part):
    """-> the listing with `; encoding: [..]` behind every instruction; the two marker comments (which llvm-mc would drop) become labels."""
    fam, k = part.split(".")
    tag = "%s_%s_%d" % (fam, k, os.getpid())
    src, enc = os.path.join(tempfile.gettempdir(), "wbc_hpb_%s.s" % tag), os.path.join(tempfile.gettempdir(), "wbc_hpb_%s.enc.s" % tag)
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S", "-g1",
                           "-D%s_PART=%s" % (fam.upper(), k), *family_flags(fam), "-DWBC_NPARTS=%d" % NPARTS.get(fam, 1)] + os.environ.get("WBC_XFLAGS", "").split()
                          + [os.path.join(CSRC, "wbc_k_%s.hip" % fam), "-o", src], stderr=subprocess.DEVNULL)
    n = [0]

    def mark(m):
        n[0] += 1
        return "%s_MARK_%d:" % (m.group(1), n[0])
    txt = re.sub(r"^\s*;\s*(WBC_COLD|WBC_TAIL_BEGIN)\s*$", mark, open(src).read(), flags=re.M)
    with open(src, "w") as f:
        f.write(txt)
    subprocess.check_call([llvm_mc(), "-triple=amdgcn-amd-amdhsa", "-mcpu=gfx950", "-show-encoding", src, "-o", enc], stderr=subprocess.DEVNULL)
    out = open(enc).read()
    os.unlink(src)
    os.unlink(enc)
    return out, [int(v) for v in re.findall(r"; codeLenInByte = (\d+)", txt)]      # (the compiler's own figure per kernel, in listing order: a comment llvm-mc drops)


MIX_CLASSES = ("fp64 arith", "mov imm", "mov reg", "select", "dpp", "other valu", "scalar", "exec-mask", "waitcnt", "nop", "lds", "global")


def classify(ins):
    """-> the --mix class of one instruction (mnemonic and operands as in the listing)"""
    mn, _, ops = ins.partition(" ")
    ops = [o.strip() for o in ops.split(",")]
    if mn.endswith("_dpp") or "row_" in ins or "quad_perm" in ins:
        return "dpp"
    if re.match(r"v_(fmac|fma|mul|add|min|max)_f64", mn):
        return "fp64 arith"
    if re.match(r"v_mov_b(32|64)", mn):
        return "mov reg" if len(ops) > 1 and re.match(r"[vsa]\d|[vsa]\[|vcc|exec|ttmp|m0", ops[1]) else "mov imm"
    if mn.startswith("v_cndmask"):
        return "select"
    if mn.startswith("v_"):
        return "other valu"
    if mn.startswith("ds_"):
        return "lds"
    if re.match(r"(global|flat|scratch|buffer)_", mn):
        return "global"
    if mn.startswith("s_waitcnt"):
        return "waitcnt"
    if mn.startswith("s_nop"):
        return "nop"
    if "saveexec" in mn or mn.startswith("s_cbranch_exec") or (ops and ops[0].startswith("exec")):
        return "exec-mask"
    return "scalar"


def analyse(part):
    """-> (part, [(kernel, hot instructions, hot bytes, span bytes, cold bytes inside the span, bytes behind the span, total)])"""
    txt, code_len = listing(part)
    res = []
    for kn, m in enumerate(re.finditer(r"^(_ZN3wbc\w+):[^\n]*\n(.*?)^\.Lfunc_end", txt, re.S | re.M)):
        name = subprocess.check_output(["c++filt", m.group(1)], text=True).strip()
        name = re.sub(r"\(.*", "", name.replace("void wbc::", ""))
        # blocks in layout order: label, start address, instructions, bytes, successors, falls through, cut (a marker inside: cold from there on)
        blocks, addr = [], 0
        cur = {"label": "entry", "start": 0, "n": 0, "bytes": 0, "hot_n": 0, "hot_bytes": 0, "sl": 0, "ss": 0, "hsl": 0, "hss": 0, "succ": [], "all_succ": [], "fall": True, "cut": False, "exit": False, "mix": [], "hot_mix": []}
        files, where = {}, "?"
        for fm in re.finditer(r'^\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', txt, re.M):
            files[fm.group(1)] = os.path.basename(fm.group(2))
        for line in m.group(2).splitlines():
            loc = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", line)
            if loc:
                where = "%s:%s" % (files.get(loc.group(1), "file" + loc.group(1)), loc.group(2))
                continue
            if re.match(r"\s*\.section", line):
                break                            # (the kernel descriptor's section follows the code)
            if re.match(r"^WBC_(COLD|TAIL_BEGIN)_MARK_\d+:", line):
                cur["cut"] = True
                continue
            lab = re.match(r"^(\.LBB\w+):", line)
            if lab:
                blocks.append(cur)
                cur = {"label": lab.group(1), "start": addr, "n": 0, "bytes": 0, "hot_n": 0, "hot_bytes": 0, "sl": 0, "ss": 0, "hsl": 0, "hss": 0, "succ": [], "all_succ": [], "fall": True, "cut": False, "exit": False, "mix": [], "hot_mix": []}
                continue
            al = re.match(r"\s*\.p2align\s+(\d+)", line)
            if al:                               # padding in front of an aligned block: counted with the block it ends
                pad = -addr % (1 << int(al.group(1)))
                addr += pad
                cur["bytes"] += pad
                continue
            e = re.search(r";\s*encoding:\s*\[([^\]]*)\]", line)
            if not e:
                continue
            nb = len(e.group(1).split(","))
            ins = line.split(";")[0].strip()
            addr += nb
            cur["n"] += 1
            cur["bytes"] += nb
            cur["mix"].append((classify(ins), where))
            sl, ss = ins.startswith("scratch_load"), ins.startswith("scratch_store")
            cur["sl"] += sl
            cur["ss"] += ss
            if not cur["cut"]:
                cur["hot_n"] += 1
                cur["hot_bytes"] += nb
                cur["hot_mix"].append(cur["mix"][-1])
                cur["hsl"] += sl
                cur["hss"] += ss
            br = re.match(r"s_(c?branch\w*)\s+(\.LBB\w+)", ins)
            if br:
                cur["all_succ"].append(br.group(2))
            if br and not cur["cut"]:
                cur["succ"].append(br.group(2))
            if br and br.group(1) == "branch":
                cur["fall"] = False
            if ins.startswith("s_endpgm") or ins.startswith("s_setpc"):
                cur["fall"] = False
                cur["exit"] = True
        blocks.append(cur)
        index = {b["label"]: i for i, b in enumerate(blocks)}

        def exits_without(c):                    # is the kernel's end reachable from its entry when block c is taken out (markers ignored)?
            seen, stack = set(), [0]
            while stack:
                i = stack.pop()
                if i in seen or i >= len(blocks) or i == c:
                    continue
                seen.add(i)
                if blocks[i]["exit"]:
                    return True
                stack.extend(index[t] for t in blocks[i]["all_succ"])
                if blocks[i]["fall"]:
                    stack.append(i + 1)
            return False
        # a marked block that no wave can get around is not a cold block: the compiler predicated a short body in line (no skip branch), every wave
        # issues it — it counts as hot
        for i, b in enumerate(blocks):
            if b["cut"] and not exits_without(i):
                b["cut"], b["succ"], b["hot_n"], b["hot_bytes"], b["hsl"], b["hss"], b["hot_mix"] = False, b["all_succ"], b["n"], b["bytes"], b["sl"], b["ss"], b["mix"]
        # a marked block with no branch in front of its marker is cold from its first instruction (the compiler hoisted the block's preamble
        # above the comment)
        for b in blocks:
            if b["cut"] and not b["succ"]:
                b["hot_n"] = b["hot_bytes"] = b["hsl"] = b["hss"] = 0
                b["hot_mix"] = []
        seen, stack = set(), [0]
        while stack:
            i = stack.pop()
            if i in seen or i >= len(blocks):
                continue
            seen.add(i)
            b = blocks[i]
            stack.extend(index[t] for t in b["succ"])        # (of a marked block: the branches in front of the marker)
            if b["fall"] and not b["cut"]:       # what lies behind a marker is reached through it
                stack.append(i + 1)
        hot_n = sum(blocks[i]["hot_n"] for i in seen)
        hot_bytes = sum(blocks[i]["hot_bytes"] for i in seen)
        last = max(i for i in seen if blocks[i]['hot_bytes'] or not blocks[i]['cut'])
        span = blocks[last]["start"] + (blocks[last]["hot_bytes"] if blocks[last]["cut"] else blocks[last]["bytes"])
        # layout map: runs of hot / cold bytes in address order (a block cut by a marker is hot up to it)
        runs = []
        for i, b in enumerate(blocks):
            for hot, nb in (((True, b["hot_bytes"]), (False, b["bytes"] - b["hot_bytes"])) if i in seen else ((False, b["bytes"]),)):
                if nb == 0:
                    continue
                if runs and runs[-1][0] == hot:
                    runs[-1][2] += nb
                else:
                    runs.append([hot, b["start"] + (0 if hot or i not in seen else b["hot_bytes"]), nb])
        scr = "%d/%d" % (sum(blocks[i]["hsl"] for i in seen), sum(blocks[i]["hss"] for i in seen))
        # self-check of the classification: the runs tile the kernel, and the kernel is as long as the compiler says
        assert sum(r[2] for r in runs) == addr and sum(r[2] for r in runs if r[0]) == hot_bytes, name
        assert code_len[kn] == addr, "%s: %d B counted, codeLenInByte = %d" % (name, addr, code_len[kn])
        mix = [x for i in sorted(seen) for x in blocks[i]["hot_mix"]]
        assert len(mix) == hot_n, name
        res.append((name, hot_n, hot_bytes, span, span - hot_bytes, addr - span, addr, scr, runs, mix))
    return part, res


def main():
    parts = [a for a in sys.argv[1:] if not a.startswith("-")] or ["sim3p.%d" % k for k in range(NPARTS["sim3p"])]
    verbose, want_mix = "-v" in sys.argv, "--mix" in sys.argv
    print("%-52s %6s %8s | %8s %8s | %8s %8s | %s" % ("kernel", "hot ins", "hot B", "span B", "inside B", "rest B", "total B", "hot scratch ld/st"))
    with ThreadPoolExecutor(max_workers=min(4, len(parts))) as ex:
        for part, res in ex.map(analyse, parts):
            for r in res:
                print("%-52s %6d %8d | %8d %8d | %8d %8d | %s" % r[:8])
                if verbose:
                    for hot, start, nb in r[8]:
                        print("      %-4s at %7d: %7d B" % ("hot" if hot else "cold", start, nb))
                if want_mix:
                    for cls in MIX_CLASSES:
                        lines = {}
                        for c, w in r[9]:
                            if c == cls:
                                lines[w] = lines.get(w, 0) + 1
                        top = sorted(lines.items(), key=lambda kv: (-kv[1], kv[0]))[:6]
                        print("      %-10s %5d   %s" % (cls, sum(lines.values()), "  ".join("%s x%d" % kv for kv in top)))


if __name__ == "__main__":
    main()
