#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assembly listings of one source file.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S pose.hip -o before.s     (at the parent)
    hipcc <the Makefile's FLAGS> --cuda-device-only -S pose.hip -o after.s      (at the change)
    python scripts/asm_kernel_diff.py before.s after.s

A kernel is its text from its `.globl` line to the next one (body, resource block, the `; NumVgprs` comments).
What names the compilation unit or counts over the whole listing is normalised: the __hip_cuid_ hash, the
`.static.<hash>` postfix, the function index in .LBB<f>_<b> / .Lfunc_end<f> / .Lfunc_begin<f>, and the running numbers of
.Ltmp<n> / .Lpost_getpc<n> (one long branch fewer in an earlier kernel renumbers every later one).  Prints every kernel
of the first listing with `same`, `DIFFERENT` (registers and spills of both) or `missing`, then the kernels only the
second has.  Exit status 1 if a kernel of the first listing differs or is missing.
"""
import re
import sys


def kernels(path):
    blocks, name, buf = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"\s*\.globl\s+(\S+)", line)
        if m or line.lstrip().startswith(".amdgpu_metadata"):
            if name is not None:
                blocks[name] = buf
            name, buf = (m.group(1) if m else None), []
        if name is not None:
            buf.append(line)
    if name is not None:
        blocks[name] = buf
    return {k: v for k, v in blocks.items() if any(l.strip() == ".end_amdhsa_kernel" for l in v)}


def norm(name, lines):
    text = "".join(lines)
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
    text = re.sub(r"\.static\.[0-9a-f]+", ".static.X", text)
    text = re.sub(r"\.L(BB|func_end|func_begin)\d+", lambda m: ".L" + m.group(1) + "F", text)
    text = re.sub(r"\.L(tmp|post_getpc)\d+", lambda m: ".L" + m.group(1) + "N", text)   # counted over the whole listing
    return text


def resources(lines):
    want = ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "Occupancy", "codeLenInByte")
    got = {}
    for line in lines:
        m = re.match(r";\s*(\w+):\s*(\d+)", line)
        if m and m.group(1) in want:
            got[m.group(1)] = int(m.group(2))
        m = re.match(r"\s*\.(sgpr|vgpr)_spill_count:\s*(\d+)", line)
        if m:
            got[m.group(1) + "_spill"] = int(m.group(2))
    return got


def key(name):
    return re.sub(r"\.static\.[0-9a-f]+", ".static.X", name)


def main(a_path, b_path):
    a = {key(k): v for k, v in kernels(a_path).items()}
    b = {key(k): v for k, v in kernels(b_path).items()}
    bad = 0
    for name, lines in a.items():
        if name not in b:
            print("missing    ", name)
            bad += 1
        elif norm(name, lines) == norm(name, b[name]):
            print("same       ", name[:150])
        else:
            print("DIFFERENT  ", name[:150])
            print("     before", resources(lines))
            print("     after ", resources(b[name]))
            bad += 1
    for name in b:
        if name not in a:
            print("new        ", name[:150], resources(b[name]))
    print(f"{len(a)} kernels before, {len(a) - bad} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
