#!/usr/bin/env python3
"""Are the kernels of two builds of one object file the same machine code?  Takes the gfx950 code object out of each host object
(.hip_fatbin, unbundled with the ROCm binutils), cuts .text at the function symbols and compares the bytes kernel by kernel (the
order of the kernels in .text follows the order of instantiation, which a refactor of the launchers may change).  No GPU.

    python tools/cmp_kernel_text.py /tmp/vx_ab_obj/values_amd/csrc/conv2d_s16.o values_amd/csrc/conv2d_s16.o

Exit status 1 if the sets of kernels differ or any kernel's bytes do."""
import os, re, subprocess, sys, tempfile
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def run(*a):
    return subprocess.check_output([os.path.join(LLVM, a[0])] + list(a[1:]), text=True)


def kernels(obj, tmp, tag):
    fat, co, txt = (os.path.join(tmp, f"{tag}.{e}") for e in ("fat", "co", "text"))
    run("llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.devnull)
    targets = [t for t in run("clang-offload-bundler", "--list", "--type=o", f"--input={fat}").split() if "gfx950" in t]
    assert len(targets) == 1, targets
    run("clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--output={co}", f"--targets={targets[0]}")
    run("llvm-objcopy", "-O", "binary", "--only-section=.text", co, txt)
    data = open(txt, "rb").read()
    m = re.search(r"\] \.text\s+PROGBITS\s+([0-9a-f]+)\s+[0-9a-f]+\s+([0-9a-f]+)", run("llvm-readelf", "-S", "-W", co))
    base = int(m.group(1), 16)
    assert int(m.group(2), 16) == len(data)
    out = {}
    for ln in run("llvm-readelf", "-s", "-W", co).splitlines():
        f = ln.split()
        if len(f) >= 8 and f[3] == "FUNC" and int(f[2]) > 0:
            off = int(f[1], 16) - base
            out[f[7]] = data[off:off + int(f[2])]
    return out


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels(sys.argv[1], tmp, "a"), kernels(sys.argv[2], tmp, "b")
    differ = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    print(f"{len(a)} / {len(b)} kernels, {sum(map(len, a.values()))} / {sum(map(len, b.values()))} bytes of kernel code, {len(differ)} differ")
    for k in differ:
        print("  ", k, "only in one" if k not in a or k not in b else f"{len(a[k])} / {len(b[k])} bytes")
    sys.exit(1 if differ else 0)
