#!/usr/bin/env python3
"""Which kernels of two source trees compile to the same machine code -- without a GPU.

    tools/compare_kernel_code.py PARENT_TREE [BRANCH_TREE]        (BRANCH_TREE defaults to this checkout)

Each tree's softwarerenderer_amd/csrc/swr_api.hip is compiled in its own csrc/ with the flags of its own `make -s print-flags` minus
the link step's, plus `--cuda-device-only -S`, once with the product's switches and once with the test build's.  Per kernel the
`.amdhsa_kernel` descriptor block and the body's text are compared, comments stripped and local labels renumbered in order of
appearance (the method of profiles/r22_cubemaps.md section 1).  Prints one JSON line per build: the kernel counts, the kernels only one
tree has, and the kernels whose text or descriptor differ.  Exit status 1 if a kernel both trees have differs."""
import json
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BUILDS = {"product": [], "test": ["-DSWR_NO_SIMPLE_SELECT", "-DSWR_WAVE_LDS_FENCE", "-DSWR_TEST_HOOKS"]}


def assembly(tree, extra, out):
    csrc = os.path.join(tree, "softwarerenderer_amd", "csrc")
    mk = subprocess.run(["make", "-s", "-C", csrc, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in mk if f != "-shared" and not f.startswith("-Wl,")]
    subprocess.run([HIPCC] + extra + flags + ["--cuda-device-only", "-S", "swr_api.hip", "-o", out], cwd=csrc, check=True,
                   capture_output=True, text=True)
    return open(out).read()


def _normalise(lines):
    names, out = {}, []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        line = re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?", lambda m: names.setdefault(m.group(0), f".L{len(names)}"), line)
        out.append(line.strip())
    return "\n".join(out)


def kernels(text):
    """{kernel: (body text, descriptor text)}"""
    lines = text.splitlines()
    desc, body = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            desc[m.group(1)] = _normalise(lines[i + 1:j])
            i = j
        m = re.match(r"^(\w+):\s*(;.*)?$", lines[i])
        if m and m.group(1) not in body:
            j = i + 1
            # (the body ends where the descriptor's section begins; .Lfunc_end follows the descriptor)
            while j < len(lines) and not re.match(r"^\.Lfunc_end\d+:|\s*\.section\b|\s*\.amdhsa_kernel\b", lines[j]):
                j += 1
            if j < len(lines):
                body[m.group(1)] = _normalise(lines[i + 1:j])
                i = j - 1
        i += 1
    return {k: (body.get(k, ""), d) for k, d in desc.items()}


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    parent = os.path.abspath(sys.argv[1])
    branch = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = False
    with tempfile.TemporaryDirectory() as tmp:
        for build, extra in BUILDS.items():
            a = kernels(assembly(parent, extra, os.path.join(tmp, f"parent_{build}.s")))
            b = kernels(assembly(branch, extra, os.path.join(tmp, f"branch_{build}.s")))
            both = sorted(set(a) & set(b))
            differ = [k for k in both if a[k] != b[k]]
            empty = [k for k in both if not a[k][0]]
            bad = bad or bool(differ) or bool(empty)
            print(json.dumps({"build": build, "kernels_parent": len(a), "kernels_branch": len(b), "identical": len(both) - len(differ),
                              "different": differ, "no_body_found": empty, "only_parent": sorted(set(a) - set(b)),
                              "only_branch": sorted(set(b) - set(a))}))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
