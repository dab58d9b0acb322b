#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libplipmi.so, unit by unit.

    python tools/isa_diff.py PARENT_BUILD_DIR BUILD_DIR      # two plip_amd/csrc/build directories

For every object file both directories hold, the gfx950 code object is unbundled and disassembled (the three commands of
tests/test_isa_audit.py::_device_asm), and the two DISASSEMBLY TEXTS are compared -- not the code objects: building the same
sources from two directories gives identical disassembly but code objects that differ in about 1 KB of path-derived identifiers.
The per-kernel metadata of `llvm-readelf --notes` (VGPR / AGPR / SGPR counts, LDS size, scratch size) is compared as well.
Prints, per unit, the number of kernels and the names of any that differ; exit status 1 if anything differs.  Runs on the CPU
with the ROCm toolchain; needs no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size")


def code_object(obj, tmp):
    """-> path of the unbundled gfx950 code object, or None for a unit without device code"""
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "unused.o")],
                       capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(fat):
        return None
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}"], check=True)
    return co if os.path.getsize(co) else None


def disassembly(co):
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    return "\n".join(l for l in text.splitlines() if "file format" not in l)


def functions(asm):
    """-> {symbol: body text}, without each line's address: a kernel that only MOVED inside its code object (another kernel of the
    unit grew) is the same kernel -- branches are relative and the encodings stay in the text"""
    out = {}
    for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M):
        out[m.group(1)] = re.sub(r"// [0-9A-F]+:", "//", m.group(2))
    return out


def metadata(co):
    """-> {kernel symbol: {field: value}} from the AMDGPU metadata note"""
    text = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        if line.lstrip().startswith("- "):     # first key of a new list entry
            cur = {}
        if cur is None:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'")
        if key in META:
            cur[key] = val
        elif key == ".symbol":                 # '<kernel>.kd'
            out[val[:-3] if val.endswith(".kd") else val] = cur
    return out


def unit(obj):
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        if co is None:
            return None
        return disassembly(co), metadata(co)


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a_dir, b_dir = argv[1], argv[2]
    names = sorted(f for f in os.listdir(a_dir) if f.endswith(".o"))
    only = sorted(set(f for f in os.listdir(b_dir) if f.endswith(".o")) ^ set(names))
    bad = bool(only)
    for f in only:
        print(f"{f}: in one build only")
    total = 0
    for f in names:
        if f in only:
            continue
        a, b = unit(os.path.join(a_dir, f)), unit(os.path.join(b_dir, f))
        if a is None or b is None:
            same = a is None and b is None
            print(f"{f}: {'no device code' if same else 'device code in one build only'}")
            bad |= not same
            continue
        (a_asm, a_meta), (b_asm, b_meta) = a, b
        fa, fb = functions(a_asm), functions(b_asm)
        differ = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
        meta_differ = sorted(k for k in set(a_meta) | set(b_meta) if a_meta.get(k) != b_meta.get(k))
        total += len(a_meta)
        if a_asm == b_asm and not meta_differ:
            print(f"{f}: {len(a_meta)} kernels, {len(fa)} symbols, {len(a_asm.splitlines())} lines of disassembly: identical")
            continue
        bad = True
        print(f"{f}: {len(a_meta)} / {len(b_meta)} kernels: {len(differ)} differ in code, {len(meta_differ)} in metadata")
        for k in differ:
            what = "missing in one build" if k not in fa or k not in fb else \
                f"{len(fa[k].splitlines())} -> {len(fb[k].splitlines())} instructions"
            print(f"    code  {k}: {what}")
        for k in meta_differ:
            print(f"    meta  {k}: {a_meta.get(k)} -> {b_meta.get(k)}")
        if not differ and a_asm != b_asm:
            print("    (text outside the functions differs)")
    print(("DIFFERENT" if bad else "IDENTICAL") + f": {len(names)} units, {total} kernels")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
