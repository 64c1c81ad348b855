#!/usr/bin/env python3
"""Resource table of ONE unit's kernels, with the code size, for comparing two trees (needs no GPU).

    python scripts/kernel_resources_unit.py [--csrc DIR] [--unit silent_pyramid_api] [substring ...]

Compiles DIR/<unit>.hip (default: this tree's pysilent_amd/csrc) for gfx950, device code only, with build.py's flags and
-Rpass-analysis=kernel-resource-usage; VGPRs / SGPRs / scratch / LDS / occupancy come from the remarks, the code size from the
kernel symbols of the code object (llvm-readelf).  `git archive <commit> pysilent_amd/csrc include | tar -x -C DIR` gives the
other tree; profiles/rgb_uint8/kernel_resources.txt is two such tables.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import build as B                  # noqa: E402
import kernel_resources as KR      # noqa: E402


def table(csrc, unit, want):
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, unit + ".o")
        r = subprocess.run([B.hipcc()] + B.FLAGS + ["--cuda-device-only", "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                    os.path.join(csrc, unit + ".hip"), "-o", obj], capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr[-3000:])
        rows = KR.parse(r.stderr)
        readelf = os.path.join(os.path.dirname(os.path.dirname(B.hipcc())), "llvm", "bin", "llvm-readelf")
        sym = subprocess.run([readelf if os.path.exists(readelf) else "llvm-readelf", "-sW", obj], capture_output=True, text=True).stdout
        size = {}
        for line in sym.split("\n"):
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC":
                size[f[7]] = int(f[2], 0)
    names = list(rows)
    lines = ["%-64s %s  code bytes" % ("kernel", "  ".join(k for _, k in KR.KEYS))]
    for mangled, name in sorted(zip(names, KR.demangle(names)), key=lambda t: t[1]):
        if want and not any(a in name for a in want):
            continue
        r = rows[mangled]
        lines.append("%-64s %s  %10d" % (name[:64], "  ".join(str(r.get(k, "-")).rjust(len(lbl)) for k, lbl in KR.KEYS),
                                       size.get(mangled, -1)))
    return lines


def main():
    args = sys.argv[1:]
    csrc, unit = os.path.join(ROOT, "pysilent_amd", "csrc"), "silent_pyramid_api"
    for flag in ("--csrc", "--unit"):
        if flag in args:
            i = args.index(flag)
            if flag == "--csrc":
                csrc = os.path.abspath(args[i + 1])
            else:
                unit = args[i + 1]
            args = args[:i] + args[i + 2:]
    print("\n".join(table(csrc, unit, args)))


if __name__ == "__main__":
    main()
