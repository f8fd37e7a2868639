#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 device code of a built library, and the comparison of two builds.

A host-only change must leave every kernel's machine code as it is.  This tool takes the code object out of a shared library's
.hip_fatbin section, disassembles it, and prints one line per kernel: a SHA-256 of its instruction text (the `// address: encoding`
comments dropped) and the resources the code object's metadata records for it.

    python tools/device_code_digest.py xpng_amd/lib/libxpng_hip.so                 # the digest
    python tools/device_code_digest.py OLD/libxpng_hip.so NEW/libxpng_hip.so      # compare; exit status 1 on any difference

In a comparison the kernels only one side has are listed, and every other kernel must be identical.  One textual difference is
tolerated and reported as such: the 32-bit literal of the s_add_u32 that directly follows an s_getpc_b64 - a PC-relative address
of a constant table, which moves when code in front of it appears or disappears.  So is one difference of layout: the run of
s_nop (and zero bytes) behind a kernel's last instruction, alignment padding that the disassembler attributes to the kernel in front of it (the
last kernel of the code object carries the padding to the end of the section, and stops carrying it when a new kernel follows).

Needs the ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-objdump, llvm-readelf) under ROCM_PATH/llvm/bin, default /opt/rocm;
names are demangled when llvm-cxxfilt or c++filt is there.  Not part of the tests or the benchmark.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".sgpr_spill_count", ".vgpr_spill_count")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def kernels_of(lib):
    """{demangled kernel name: (instruction lines, tolerant instruction lines, {metadata field: value})}"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, elf = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.elf")
        run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib)
        run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + elf)
        asm = run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", elf)
        notes = run("llvm-readelf", "--notes", elf)
    meta, cur = {}, None
    for line in notes.splitlines():
        if line.startswith("  - ."):  # a new entry of amdhsa.kernels
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    (\.\w+): +(\S+)$", line)
        if cur is not None and m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                meta[m.group(2)] = cur
    text, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"<(\S+)>:$", line)
        if m:
            name = m.group(1)
            text[name] = []
        elif name and line.startswith("\t"):
            text[name].append(re.sub(r"\s*//.*$", "", line).strip())
    names = sorted(n for n in text if n in meta)
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")  # (neither: the mangled names serve as well)
    demangled = subprocess.run([filt, *names], check=True, capture_output=True, text=True).stdout.splitlines() if filt else names
    out = {}
    for n, d in zip(names, demangled):
        lines = text[n]
        tolerant = [re.sub(r"0x[0-9a-f]+$", "<pc-relative>", l) if i and lines[i - 1].startswith("s_getpc_b64") and l.startswith("s_add_u32") else l
                    for i, l in enumerate(lines)]
        out[d] = (lines, tolerant, {f: meta[n].get(f, "-") for f in FIELDS})
    return out


def unpadded(lines):
    """without the s_nop alignment padding behind the last instruction"""
    n = len(lines)
    while n and lines[n - 1] in ("s_nop 0", "..."):  # ("...": the disassembler's mark for a run of zero bytes, the section's very end)
        n -= 1
    return lines[:n]


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def digest(lib):
    ks = kernels_of(lib)
    print(f"# {lib}: {len(ks)} kernels; sha256/16 of the instruction text, instructions, " + " ".join(f[1:] for f in FIELDS))
    for d, (lines, _, m) in sorted(ks.items()):
        print(sha(lines), len(lines), " ".join(m[f] for f in FIELDS), d)
    return ks


def main(argv):
    if len(argv) == 2:
        digest(argv[1])
        return 0
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = digest(argv[1]), digest(argv[2])
    bad = 0
    for d in sorted(set(a) - set(b)):
        print("ONLY IN", argv[1] + ":", d)
    for d in sorted(set(b) - set(a)):
        print("ONLY IN", argv[2] + ":", d)
    for d in sorted(set(a) & set(b)):
        if a[d][2] != b[d][2]:
            print("RESOURCES DIFFER:", d, a[d][2], b[d][2])
            bad += 1
        if a[d][0] == b[d][0]:
            continue
        if a[d][1] == b[d][1]:
            print("identical up to a PC-relative literal behind s_getpc_b64:", d)
        elif unpadded(a[d][1]) == unpadded(b[d][1]):
            print(f"identical up to the s_nop padding behind its end ({len(a[d][0]) - len(unpadded(a[d][0]))} -> {len(b[d][0]) - len(unpadded(b[d][0]))} padding lines):", d)
        else:
            print("CODE DIFFERS:", d)
            bad += 1
    print(f"# {len(set(a) & set(b))} kernels in both, {bad} differ; {len(set(a) - set(b))} only in the first, {len(set(b) - set(a))} only in the second")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
