#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same, kernel for kernel? For a refactor that must not touch device code: compares, over every gfx950
code object of two libraries (or object files), the set of kernel descriptors (.kd symbols), each function's disassembly (mnemonics, operands
and encodings; the address column is dropped, so a function may sit elsewhere in its code object) and each kernel's metadata note (registers,
LDS, scratch, spill counts, kernarg layout). Code objects are not compared byte for byte: every compilation names a __hip_cuid_<hash> symbol
of its own. Prints the verdict; exit status 1 on any difference. Needs no GPU.
--mnemonics: for a function whose ISA differs, also say whether the multiset of its mnemonics is equal (then the two differ in register names,
operands and order at most) or which mnemonics it gained and lost.
usage: tools/same_kernels.py [--mnemonics] old/libwbc_hip.so new/libwbc_hip.so"""
import collections
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


def mnemonics(text):
    """-> the multiset of a function's mnemonics: what stays of its ISA when register names, operands and order are set aside"""
    return collections.Counter(line.split()[0] for line in text.splitlines())


def isa_finding(old, new, with_mnemonics):
    what = "ISA differs (%d vs %d instructions" % (old.count("\n") + 1, new.count("\n") + 1)
    if with_mnemonics:
        a, b = mnemonics(old), mnemonics(new)
        delta = ["%s %+d" % (m, b[m] - a[m]) for m in sorted(set(a) | set(b)) if a[m] != b[m]]
        what += "; mnemonic multiset " + ("EQUAL" if not delta else "differs: " + ", ".join(delta))
    return what + ")"


def main():
    args = [a for a in sys.argv[1:] if a != "--mnemonics"]
    if len(args) != 2:
        sys.exit(__doc__)
    with_mnemonics = len(args) != len(sys.argv) - 1
    (fa, ma, ka, na), (fb, mb, kb, nb) = kernels(args[0]), kernels(args[1])
    bad = [("kernel only in old", n) for n in sorted(ka - kb)] + [("kernel only in new", n) for n in sorted(kb - ka)]
    bad += [("function only in %s" % ("old" if n in fa else "new"), n) for n in sorted(set(fa) ^ set(fb))]
    bad += [(isa_finding(fa[n], fb[n], with_mnemonics), n) for n in sorted(set(fa) & set(fb)) if fa[n] != fb[n]]
    bad += [("metadata note %s" % ("differs" if n in ma and n in mb else "missing on one side"), n) for n in sorted(set(ma) | set(mb)) if ma.get(n) != mb.get(n)]
    if bad:
        for (what, _), nice in zip(bad, kr.demangle([n for _, n in bad])):
            print("%s: %s" % (what, nice))
    print("old: %d code objects, %d kernels, %d functions; new: %d code objects, %d kernels, %d functions" % (na, len(ka), len(fa), nb, len(kb), len(fb)))
    print("DIFFERENT: %d findings" % len(bad) if bad else "SAME: identical kernel set, ISA and metadata notes for all %d kernels" % len(ka))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
