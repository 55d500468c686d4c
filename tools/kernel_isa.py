#!/usr/bin/env python3
"""Per-kernel resources and an instruction-stream digest of the gfx950 code in object files or libraries built by
neuroquant_amd/csrc/Makefile -- to show, without a GPU, that a source change left a kernel's machine code alone.

    python tools/kernel_isa.py neuroquant_amd/csrc/build/conv_igemm3_k3.o [more .o / .so ...] [--match igemm3] [--strip-arg false]

One line per kernel: demangled name, VGPRs, SGPRs, bytes of scratch, spilled VGPRs, instruction count and the SHA-256 (first 16
hex digits) of its disassembly with addresses and encodings removed.  Two builds agree on a kernel when their lines agree: run it on
the objects of two checkouts and diff the outputs.  --strip-arg X drops every trailing template argument X from the printed
names, for comparing against a build from before defaulted template parameters were added (give it to both builds).
Uses llvm-objcopy, clang-offload-bundler, llvm-objdump and llvm-readelf of $ROCM_PATH/lib/llvm/bin (default /opt/rocm) and
c++filt from the PATH."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def code_object(path, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    run("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat)
    run("clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--targets={TARGET}", f"--output={co}")
    return co


def kernels(path):
    """{mangled name: dict(vgpr, sgpr, scratch, spill, n, sha)}"""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(path, tmp)
        notes, dis = run("llvm-readelf", "--notes", co), run("llvm-objdump", "-d", co)
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        out[g("name")] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), scratch=int(g("private_segment_fixed_size")),
                              spill=int(g("vgpr_spill_count")))
    name, body = None, []

    def close():
        if name in out:
            out[name].update(n=len(body), sha=hashlib.sha256("\n".join(body).encode()).hexdigest()[:16])

    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            close()
            name, body = m.group(1), []
        elif ln.startswith("\t") and name is not None:
            body.append(ln.split("//")[0].strip())      # the text of the instruction: no address, no encoding
    close()
    return out


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="+")
    ap.add_argument("--match", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--strip-arg", default=None, help="drop every trailing occurrence of this template argument from the names")
    a = ap.parse_args(argv)
    for path in a.files:
        ks = kernels(path)
        filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")     # without one the names stay mangled
        names = subprocess.run([filt, *ks], check=True, capture_output=True, text=True).stdout.splitlines() if filt and ks else list(ks)
        rows = []
        for (mangled, k), nm in zip(ks.items(), names):
            nm = nm.replace("(anonymous namespace)::", "")
            nm = nm[5:] if nm.startswith("void ") else nm
            nm = nm[:nm.rindex(">(") + 1] if ">(" in nm else nm.split("(")[0]      # without the argument list
            if a.strip_arg:
                nm = re.sub(r"(,\s*" + re.escape(a.strip_arg) + r")+>$", ">", nm)
            if a.match in nm and "n" in k:
                rows.append(f"{nm}  vgpr {k['vgpr']} sgpr {k['sgpr']} scratch {k['scratch']} spill {k['spill']} "
                            f"insts {k['n']} sha {k['sha']}")
        print(f"== {os.path.basename(path)}: {len(rows)} kernels")
        print("\n".join(sorted(rows)))


if __name__ == "__main__":
    main(sys.argv[1:])
