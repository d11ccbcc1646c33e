#!/usr/bin/env python3
"""Registers, static LDS and scratch of every kernel in a built library, from the code objects' metadata notes -- no GPU needed.

    tools/kernel_resources.py chromap_amd/libchromap_amd.so                 one JSON object: kernel -> numbers
    tools/kernel_resources.py BEFORE.so AFTER.so                            the kernels whose numbers differ, both values

The library's .hip_fatbin section holds one clang offload bundle per source file; every gfx950 code object of every bundle is
read with llvm-readelf --notes.  Waves per SIMD follow from the VGPR count (512 registers per lane, allocated in blocks of 8,
at most 8 waves)."""
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KEYS = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".group_segment_fixed_size": "lds",
        ".private_segment_fixed_size": "scratch", ".vgpr_spill_count": "vgpr_spill", ".sgpr_spill_count": "sgpr_spill"}


def waves_per_simd(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def code_objects(lib, arch):
    with tempfile.TemporaryDirectory() as tmp:
        sec = os.path.join(tmp, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + sec, lib, os.path.join(tmp, "copy")])
        blob = open(sec, "rb").read()
    at = blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if triple.endswith(arch) and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + len(MAGIC))


def resources(lib, arch="gfx950"):
    out = {}
    for co in code_objects(lib, arch):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], text=True)
        cur = None
        for line in notes.splitlines():
            m = re.match(r"\s*-?\s*(\.[a-z_]+):\s*(.*)$", line)
            if not m:
                continue
            key, val = m.group(1), m.group(2).strip().strip("'")
            if line.lstrip().startswith("- ") and key in KEYS.keys() | {".name", ".agpr_count", ".args"}:
                cur = {}  # a new kernel's record (its first key; .name follows)
            if cur is None:
                continue
            if key in KEYS:
                cur[KEYS[key]] = int(val)
            elif key == ".symbol" and val.endswith(".kd"):
                out[val[:-3]] = cur
    for r in out.values():
        r["waves_per_simd"] = waves_per_simd(r.get("vgpr", 0) + r.get("agpr", 0))
    return out


def demangled(table):
    """the table with its kernel names demangled (one filter process for all of them)"""
    names = list(table)
    for tool in (os.path.join(LLVM, "llvm-cxxfilt"), "c++filt"):
        try:
            plain = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
            return {p: table[n] for p, n in zip(plain, names)}
        except (OSError, subprocess.CalledProcessError):
            pass
    return table


if __name__ == "__main__":
    if len(sys.argv) == 2:
        print(json.dumps(demangled(resources(sys.argv[1])), indent=1, sort_keys=True))
    else:
        a, b = resources(sys.argv[1]), resources(sys.argv[2])
        diff = {k: {"before": a.get(k), "after": b.get(k)} for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)}
        print(json.dumps({"kernels": [len(a), len(b)], "changed": demangled(diff)}, indent=1, sort_keys=True))
