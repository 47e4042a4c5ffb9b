#!/usr/bin/env python3
"""Do two builds of a library hold the same kernels, instruction for instruction?  `kernel_code_diff.py OLD.so NEW.so`

Every gfx950 code object of both libraries is extracted (kernel_resources.code_objects) and disassembled; the text is cut
per function symbol, so a kernel may move to another translation unit between the two builds. Two things are not compared,
because they depend on where the linker put a function and not on its code: the padding behind a function, and the
literal of the s_add_u32 / s_addc_u32 that follows an s_getpc_b64 (a pc-relative address of constant data). Prints one
line per symbol, `same` or `differs` with the instruction counts, and exits non-zero if any differs or exists on one side
only. A symbol defined in several code objects (the weak instantiations of library templates) counts once per definition."""
import os
import re
import subprocess
import sys
import tempfile

import kernel_resources as kr

PADDING = re.compile(r"^(s_nop 0|s_code_end|\.\.\.)$")


def kernel_code(lib):
    """{symbol: sorted list of instruction tuples, one per definition} over all gfx950 code objects of `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in kr.code_objects(lib, d):
            text = subprocess.run([os.path.join(kr.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                  capture_output=True, text=True, check=True).stdout
            cur, pc = None, 0  # pc: how many of the two additions behind an s_getpc_b64 may still follow
            for line in text.splitlines():
                m = re.match(r"^<(.+)>:$", line)
                if m:
                    cur, pc = [], 0
                    out.setdefault(m.group(1), []).append(cur)
                    continue
                ins = " ".join(line.split("//")[0].split())  # (the address and the encoding stand in a trailing comment)
                if cur is None or not ins:
                    continue
                if ins.startswith("s_getpc_b64"):
                    pc = 2
                elif pc and re.match(r"s_addc?_u32 ", ins):
                    ins, pc = ins.rsplit(",", 1)[0] + ", <pc-relative>", pc - 1
                else:
                    pc = 0
                cur.append(ins)
    for defs in out.values():
        for body in defs:
            while body and PADDING.match(body[-1]):
                body.pop()
    return {n: sorted(tuple(b) for b in defs) for n, defs in out.items()}


def diff(old, new):
    """(report lines, number of symbols that differ or exist on one side only) of two kernel_code() results."""
    names = sorted(set(old) | set(new))
    short = kr._demangle(names)
    count = lambda defs: "+".join(str(len(x)) for x in defs) if defs else "-"
    lines, bad = [], 0
    for n in names:
        a, b = old.get(n), new.get(n)
        verdict = "same" if a == b else "differs" if a and b else "only old" if a else "only new"
        bad += a != b
        lines.append("%-8s %8s %8s  %s" % (verdict, count(a), count(b), re.sub(r"\(.*$", "", short[n])[:160]))
    lines.append("%d symbols, %d same, %d differ or exist on one side only" % (len(names), len(names) - bad, bad))
    return lines, bad


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    lines, bad = diff(kernel_code(sys.argv[1]), kernel_code(sys.argv[2]))
    print("\n".join(lines))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
