#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same, kernel for kernel? For a refactor that must not touch device code: compares, over every gfx950
code object of two libraries (or object files), the set of kernel descriptors (.kd symbols), each function's disassembly (mnemonics, operands
and encodings; the address column is dropped, so a function may sit elsewhere in its code object) and each kernel's metadata note (registers,
LDS, scratch, spill counts, kernarg layout). Code objects are not compared byte for byte: every compilation names a __hip_cuid_<hash> symbol
of its own. Prints the verdict; exit status 1 on any difference. Needs no GPU.
usage: tools/same_kernels.py old/libwbc_hip.so new/libwbc_hip.so"""
import re
import subprocess
import sys
import tempfile

import kernel_resources as kr


def kernels(path):
    """-> ({function: disassembly without addresses}, {kernel: metadata note}, {names of the .kd symbols}, number of code objects)"""
    funcs, meta, kds = {}, {}, set()
    cos = kr.code_objects(path)
    for elf in cos:
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(elf)
            f.flush()
            dis = subprocess.check_output([kr.LLVM + "/llvm-objdump", "-d", f.name], text=True)
            syms = subprocess.check_output([kr.LLVM + "/llvm-readelf", "--symbols", "--wide", f.name], text=True)
        kds.update(re.findall(r"(\S+)\.kd$", syms, re.M))
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                assert cur not in funcs, "function %s in two code objects" % cur
                funcs[cur] = []
            elif cur and line.strip():
                funcs[cur].append(re.sub(r"// [0-9A-Fa-f]+:", "//", re.sub(r"<[^>]*>", "", line)).strip())
        for blk in re.split(r"\n\s*- \.agpr_count", kr.notes(elf))[1:]:
            blk = re.split(r"\n\s*amdhsa\.target", blk)[0]
            meta[re.search(r"\.name:\s*(\S+)", blk).group(1)] = blk
    return {k: "\n".join(v) for k, v in funcs.items()}, meta, kds, len(cos)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (fa, ma, ka, na), (fb, mb, kb, nb) = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = [("kernel only in old", n) for n in sorted(ka - kb)] + [("kernel only in new", n) for n in sorted(kb - ka)]
    bad += [("function only in %s" % ("old" if n in fa else "new"), n) for n in sorted(set(fa) ^ set(fb))]
    bad += [("ISA differs (%d vs %d instructions)" % (fa[n].count("\n") + 1, fb[n].count("\n") + 1), n) for n in sorted(set(fa) & set(fb)) if fa[n] != fb[n]]
    bad += [("metadata note %s" % ("differs" if n in ma and n in mb else "missing on one side"), n) for n in sorted(set(ma) | set(mb)) if ma.get(n) != mb.get(n)]
    if bad:
        for (what, _), nice in zip(bad, kr.demangle([n for _, n in bad])):
            print("%s: %s" % (what, nice))
    print("old: %d code objects, %d kernels, %d functions; new: %d code objects, %d kernels, %d functions" % (na, len(ka), len(fa), nb, len(kb), len(fb)))
    print("DIFFERENT: %d findings" % len(bad) if bad else "SAME: identical kernel set, ISA and metadata notes for all %d kernels" % len(ka))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
