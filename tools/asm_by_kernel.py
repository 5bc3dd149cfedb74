#!/usr/bin/env python3
"""Device assembly of one translation unit in a form two builds can be diffed in: kernels sorted by symbol.

The compiler emits template instances in the order the host code first names them, and numbers local labels by that order, so a
change of host code alone reorders and renumbers an otherwise identical file.  This prints every function's text section with the
`.amdhsa_kernel` block that follows it and every kernel's entry of the metadata note, each sorted by symbol, with comments, `.file` /
`.ident` lines and the per-function label numbers (`.LBB12_3`, `.Lfunc_end12`) taken out.

    hipcc $CXXFLAGS --cuda-device-only -S csrc/deform.hip -o new.s        (CXXFLAGS of csrc/Makefile; the same for the other build)
    diff <(python tools/asm_by_kernel.py old.s) <(python tools/asm_by_kernel.py new.s)
"""
import re
import sys


def normalised(path):
    lines = []
    for line in open(path):
        line = line.split(";")[0].rstrip()
        if line.strip() and not re.match(r"\s*\.(file|ident)\b", line):
            line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)          # (a hash of the source text)
            lines.append(re.sub(r"\.L(BB|func_(?:begin|end)|tmp)\d+", r".L\1", line))
    text = "\n".join(lines)
    head, *funcs = re.split(r"\n(?=\t\.section\t\.text\.)", text)
    funcs[-1], middle, note = re.split(r"\n(?=\t\.section\t\.AMDGPU\.gpr_maximums|\t\.amdgpu_metadata)", funcs[-1])
    first, *kernels = re.split(r"\n(?=\s*- \.agpr_count)", note)
    kernels[-1], tail = re.split(r"\n(?=amdhsa\.target)", kernels[-1])
    return "\n".join([head] + sorted(funcs) + [middle, first] + sorted(kernels) + [tail]) + "\n"


if __name__ == "__main__":
    sys.stdout.write(normalised(sys.argv[1]))
