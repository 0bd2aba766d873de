#!/usr/bin/env python3
"""Do two builds hold the same kernels?  For every kernel of every object (build/*.o) of two build directories: the number of
instructions in each, SAME / DIFF of the disassembled instruction streams as text (addresses, encodings and branch targets stripped),
and vgpr / spill / scratch / LDS of both from the code-object metadata (tools/kernel_resources.py).

    python tools/kernel_stream_diff.py BUILD_A BUILD_B [substring]

A refactor of a kernel header is checked by building the parent commit into a directory of its own and comparing the two.

The comparison is of the text, line by line, after three kinds of address have been taken out: the address and encoding that
the disassembler prints behind each instruction, the numbers of branch targets (L12 -> L), and the pc-relative address of a constant
in .rodata.  The last is an ordinary literal operand whose value depends on how much code lies in front of the instruction, so
a kernel that did not change would differ whenever one before it in the object grew.  The rule is by value, not by instruction: a hex
literal is rewritten as <.rodata+offset> iff the instruction's own address plus the literal lies inside .rodata.  Two literals then
still compare unequal unless they name the same byte of .rodata; a literal that is no address is taken for one only if it happens
to equal the distance from its instruction to .rodata (for these objects: 0xff......), and it could hide a difference only if the
other build's literal differs by exactly the amount the code moved.  A kernel whose stream is empty in either build is an error
(EMPTY), never SAME; the exit status is 1 then.
"""
import os
import re
import subprocess
import sys
import tempfile

import kernel_resources as kr


def streams(co):
    """{symbol: [instruction text]} of a code object"""
    objdump = os.path.join(kr.LLVM, "llvm-objdump")
    # .rodata: a literal that, added to its instruction's own address, points into it is written as section + offset (see above)
    heads = subprocess.run([objdump, "-h", co], capture_output=True, text=True, check=True).stdout
    data = [(m.group(1), int(m.group(3), 16), int(m.group(2), 16)) for m in re.finditer(r"^\s*\d+\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+DATA$", heads, re.M) if m.group(1) == ".rodata"]

    def literal(m, addr):
        t = (addr + int(m.group(0), 16)) & 0xFFFFFFFF
        for name, vma, size in data:
            if vma <= t < vma + size:
                return "<%s+%#x>" % (name, t - vma)
        return m.group(0)

    dis = subprocess.run([objdump, "-d", "--symbolize-operands", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            if not re.fullmatch(r"L\d+", m.group(1)):         # a branch target inside the current function is not a new one
                cur = out.setdefault(m.group(1), [])
        elif line.startswith("\t") and cur is not None:
            text, _, comment = line.partition("//")
            at = re.match(r"\s*([0-9A-Fa-f]+):", comment)     # the instruction's address leads the disassembler's comment
            if at:
                text = re.sub(r"\b0x[0-9a-f]+\b", lambda m: literal(m, int(at.group(1), 16)), text)
            cur.append(re.sub(r"\bL\d+\b", "L", text.strip()))
    return out


def kernels(build):
    """{(object, symbol): (instruction stream, metadata fields)}"""
    out = {}
    for fn in kr.objects(build):
        with tempfile.TemporaryDirectory() as td:
            co = kr.code_object(os.path.join(build, fn), td)
            if co is None:
                continue
            st = streams(co)
            for symbol, fields in kr.kernel_metadata(co):
                out[(fn, symbol)] = (st.get(symbol, []), fields)
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = sys.argv[3] if len(sys.argv) > 3 else ""
    want = (0, 1, 3, 4)                                       # vgpr, spill, scratch, LDS of kr.FIELDS
    print("%-14s %-90s %7s %7s %-5s %s" % ("object", "kernel", "insts A", "insts B", "", "vgpr/spill/scratchB/ldsB A -> B"))
    ndiff = empty = 0
    for key in sorted(set(a) | set(b)):
        name = kr.demangle(key[1])
        if pat not in name:
            continue
        (sa, fa), (sb, fb) = a.get(key, ([], None)), b.get(key, ([], None))
        verdict = "ONLY A" if not fb else "ONLY B" if not fa else "EMPTY" if not sa or not sb else "SAME" if sa == sb else "DIFF"
        ndiff += verdict != "SAME"
        empty += verdict == "EMPTY"
        res = " -> ".join("/".join(f[i] for i in want) if f else "-" for f in (fa, fb))
        print("%-14s %-90s %7d %7d %-5s %s" % (key[0], name, len(sa), len(sb), verdict, res))
    print("%d kernels differ" % ndiff)
    if empty:
        sys.exit("%d kernels have no disassembly" % empty)


if __name__ == "__main__":
    main()
