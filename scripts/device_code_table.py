#!/usr/bin/env python3
"""scripts/device_code_table.py <objects of build A> <objects of build B> [--table FILE] — compares the DEVICE code of two builds of
the library without a GPU. For every unit (`*.o` of a `make OBJ=…` directory) the gfx950 code object is taken out of the fat binary
(`llvm-objcopy --dump-section .hip_fatbin`, `clang-offload-bundler --unbundle`), then:

  * the SHA-256 of its `.text` (`llvm-objcopy -O binary --only-section=.text`) — equal hashes: the same machine code;
  * per kernel, the code bytes (`llvm-readelf -sW`) and what the code object's metadata records (`llvm-readelf --notes`): VGPRs,
    AGPRs, SGPRs, spilled VGPRs and SGPRs, scratch bytes per lane, LDS bytes, and the waves per SIMD that leaves room for
    (512 registers per SIMD lane, VGPRs + AGPRs in units of 8, at most 8 waves).

Prints one line per unit and, with --table, writes the per-kernel table of the kernels that differ in any column (or of all of
them, --all). Exit status 1 if a kernel of B is larger or differs in a resource column."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
COLUMNS = ("bytes", "vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds", "waves")


def run(*command):
    return subprocess.run(command, check=True, capture_output=True, text=True).stdout


def device_elf(object_path, directory):
    fatbin = os.path.join(directory, "fatbin")
    elf = os.path.join(directory, "device.elf")
    run(f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fatbin}", object_path)
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fatbin}", f"--output={elf}",
        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950")
    return elf


def unit(object_path):
    """(hash of .text, {kernel: {column: value}})"""
    with tempfile.TemporaryDirectory() as directory:
        elf = device_elf(object_path, directory)
        text = os.path.join(directory, "text")
        run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.text", elf, text)
        digest = hashlib.sha256(open(text, "rb").read()).hexdigest()
        sizes = {}
        for line in run(f"{LLVM}/llvm-readelf", "-sW", elf).splitlines():
            fields = line.split()
            if len(fields) == 8 and fields[3] == "FUNC":
                sizes[fields[7]] = int(fields[2], 0)
        kernels = {}
        for block in run(f"{LLVM}/llvm-readelf", "--notes", elf).split("- .agpr_count:")[1:]:
            def field(key, block=block):
                found = re.search(r"\." + key + r":\s+(\d+)", block)
                return int(found.group(1)) if found else 0
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            agpr = int(block.split()[0])
            vgpr = field("vgpr_count")  # on gfx950 the unified count: VGPRs and AGPRs of one budget
            waves = min(8, 512 // max(8, (vgpr + 7) // 8 * 8))
            kernels[name] = dict(bytes=sizes.get(name, 0), vgpr=vgpr, agpr=agpr, sgpr=field("sgpr_count"),
                                 vgpr_spill=field("vgpr_spill_count"), sgpr_spill=field("sgpr_spill_count"),
                                 scratch=field("private_segment_fixed_size"), lds=field("group_segment_fixed_size"), waves=waves)
        return digest, kernels


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("a")
    parser.add_argument("b")
    parser.add_argument("--table")
    parser.add_argument("--all", action="store_true")
    parser.add_argument("--units", default="search_,test_hooks", help="prefixes of the units to compare")
    options = parser.parse_args()
    prefixes = tuple(options.units.split(","))
    names = sorted(n for n in os.listdir(options.a) if n.endswith(".o") and n.startswith(prefixes))
    rows, worse = [], False
    for name in names:
        if not os.path.exists(os.path.join(options.b, name)):
            continue
        try:
            (hash_a, kernels_a), (hash_b, kernels_b) = unit(os.path.join(options.a, name)), unit(os.path.join(options.b, name))
        except subprocess.CalledProcessError:
            continue  # a unit without device code
        changed = 0
        for kernel in sorted(set(kernels_a) | set(kernels_b)):
            a, b = kernels_a.get(kernel), kernels_b.get(kernel)
            differs = a != b
            changed += differs
            if a is None or b is None or b["bytes"] > a["bytes"] or any(a[c] != b[c] for c in COLUMNS[1:]):
                worse = True
            if differs or options.all:
                rows.append((name[:-2], kernel, a, b))
        print(f"{name[:-2]:28s} kernels {len(kernels_b):4d}  .text {'EQUAL' if hash_a == hash_b else 'differs'}  "
              f"{hash_a[:16]} {hash_b[:16]}  kernels that differ {changed}", flush=True)
    if options.table:
        with open(options.table, "w") as out:
            out.write("# unit kernel | A: " + " ".join(COLUMNS) + " | B: the same\n")
            for name, kernel, a, b in rows:
                cells = lambda k: " ".join(str(k[c]) for c in COLUMNS) if k else "absent"
                out.write(f"{name} {kernel} | {cells(a)} | {cells(b)}\n")
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
