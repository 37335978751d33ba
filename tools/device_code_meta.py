#!/usr/bin/env python3
"""Per-kernel metadata of the gfx950 code objects inside a built library, and the comparison of two
libraries: the evidence that a host-side change left the device code alone.

  python tools/device_code_meta.py LIB            # one line per kernel
  python tools/device_code_meta.py LIB_A LIB_B    # compare; exit status 1 if anything differs

For every kernel: vgpr / sgpr count, LDS (group segment) and scratch (private segment) size, spill
counts (the code object's metadata notes) and the code size (the kernel's function symbol).  A kernel
name that occurs in more than one code object of a library is reported: it was compiled twice.
"""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("SLG_LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".vgpr_spill_count", ".sgpr_spill_count")


def code_objects(lib, tmp):
    """the gfx950 code objects of every offload bundle in the library's .hip_fatbin section"""
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib,
                           os.path.join(tmp, "discard.so")])
    data = open(fat, "rb").read()
    out = []
    pos = data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                path = os.path.join(tmp, "co%d.elf" % len(out))
                open(path, "wb").write(data[pos + off:pos + off + size])
                out.append(path)
        pos = data.find(MAGIC, pos + 1)
    if not out:
        raise SystemExit("%s: no uncompressed gfx950 code object found in .hip_fatbin" % lib)
    return out


def kernels(lib):
    """{kernel name: [metadata dict per occurrence]}"""
    found = collections.defaultdict(list)
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            sizes = {}
            syms = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-s", "-W", co], text=True)
            for line in syms.splitlines():
                f = line.split()
                if len(f) >= 8 and f[3] == "FUNC":
                    sizes[f[7]] = int(f[2], 0)
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
            # amdhsa.kernels: one map per kernel, opened by "  - "; its own keys are indented by four
            # (deeper ones describe arguments)
            recs, in_kernels = [], False
            for line in notes.splitlines():
                if not line.startswith(" "):
                    in_kernels = line.startswith("amdhsa.kernels:")
                    continue
                m = re.match(r"  (- |  )(\.[a-z_]+):\s*(.*)$", line)
                if not in_kernels or not m:
                    continue
                if m.group(1) == "- ":
                    recs.append({})
                recs[-1][m.group(2)] = m.group(3).strip().strip("'\"")
            for r in recs:
                rec = {k: r.get(k) for k in FIELDS}
                rec["code_bytes"] = sizes.get(r[".name"])
                found[r[".name"]].append(rec)
    return found


def fmt(rec):
    return " ".join("%s=%s" % (k.lstrip("."), rec[k]) for k in FIELDS + ("code_bytes",))


def main(argv):
    if len(argv) == 2:
        for name, recs in sorted(kernels(argv[1]).items()):
            for r in recs:
                print(name, fmt(r))
        return 0
    a, b = kernels(argv[1]), kernels(argv[2])
    bad = 0
    print("A = %s: %d kernel names; B = %s: %d kernel names" % (argv[1], len(a), argv[2], len(b)))
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("ONLY IN %s: %s" % ("A" if name in a else "B", name))
            bad += 1
        elif len(a[name]) != len(b[name]):
            print("COMPILED %d TIMES IN A, %d IN B: %s" % (len(a[name]), len(b[name]), name))
            bad += 1
        elif [fmt(r) for r in a[name]] != [fmt(r) for r in b[name]]:
            print("DIFFERS: %s\n  A %s\n  B %s" % (name, "; ".join(map(fmt, a[name])), "; ".join(map(fmt, b[name]))))
            bad += 1
    print("%d kernel names compared, %d differences" % (len(set(a) | set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        raise SystemExit(__doc__)
    sys.exit(main(sys.argv))
