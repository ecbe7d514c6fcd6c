#!/usr/bin/env python3
"""Do two builds give a kernel the same instructions?

    make -C audiotoken_amd/csrc build/NAME.s          (in both checkouts)
    python tools/asm_same.py OLD_BUILD_DIR NEW_BUILD_DIR NAME.s OLD_KERNEL_REGEX [NEW_KERNEL_REGEX]

Compares the instruction streams of the kernels whose (mangled) names match the regular expressions, comments and assembler directives removed
and local labels renumbered (their numbers count the functions of the file). Prints the instruction counts, the register / LDS figures of the
kernel descriptors and IDENTICAL or the first differing lines; the exit status is 0 only when the streams are identical.
"""
import re
import sys


def kernel(path, pattern):
    txt = open(path).read()
    hits = [m for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)\n\s*\.end_amdhsa_kernel", txt, re.S | re.M) if re.search(pattern, m.group(1))]
    if len(hits) != 1:
        raise SystemExit(f"{path}: {len(hits)} kernels match {pattern!r}: {[m.group(1) for m in hits]}")
    name, body = hits[0].group(1), hits[0].group(2)
    code = body.split(".section")[0]
    lines = [re.sub(r"\s*;.*", "", ln).rstrip() for ln in code.splitlines()]
    lines = [re.sub(r"\.LBB\d+_", ".LBB_", ln) for ln in lines if ln.strip() and not ln.strip().startswith(".")]
    meta = dict(re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size)\s+(\S+)", body))
    return name, lines, meta


def main():
    old_dir, new_dir, fname, old_re = sys.argv[1:5]
    new_re = sys.argv[5] if len(sys.argv) > 5 else old_re
    n0, a, m0 = kernel(f"{old_dir}/{fname}", old_re)
    n1, b, m1 = kernel(f"{new_dir}/{fname}", new_re)
    same = a == b
    print(f"{fname}: {n0}\n{'':{len(fname)}s}  -> {n1}\n  instructions {len(a)} -> {len(b)}, descriptor {m0} -> {m1}: {'IDENTICAL' if same and m0 == m1 else 'DIFFERENT'}")
    if not same:
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                print(f"  first difference at instruction {i}:\n    - {x}\n    + {y}")
                break
    sys.exit(0 if same and m0 == m1 else 1)


if __name__ == "__main__":
    main()
