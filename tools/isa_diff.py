#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libplipmi.so, kernel by kernel.

    python tools/isa_diff.py PARENT_BUILD_DIR BUILD_DIR      # two plip_amd/csrc/build directories

For every object file of either directory, the gfx950 code object is unbundled and disassembled (the three commands of
tests/test_isa_audit.py::_device_asm), and the two DISASSEMBLY TEXTS are compared -- not the code objects: building the same
sources from two directories gives identical disassembly but code objects that differ in about 1 KB of path-derived identifiers.
The per-kernel metadata of `llvm-readelf --notes` (VGPR / AGPR / SGPR counts, LDS size, scratch size) is compared as well.

Kernels are matched BY SYMBOL over all units, so a kernel that moved to another translation unit is compared with itself; the
report names the unit it came from.  A kernel whose only difference is the literal of the s_add_u32 / s_addc_u32 pair directly
after an s_getpc_b64 -- the pc-relative address of the unit's constant data, which moves whenever a kernel in front of it
changes size or the unit's set of kernels changes -- is listed as "constant address only" and does not count as different.
Prints, per unit of BUILD_DIR, the number of kernels and the names of any that differ; exit status 1 if a kernel differs in
anything else, exists in one build only, or is defined by two units of one build (only one of the two bodies is compared).  Runs on the CPU with the ROCm toolchain; needs no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size")


PADDING = re.compile(r"\s*(?:(?:s_nop 0|s_code_end)\s*//.*|\.\.\.)?$")   # a line after a kernel's last instruction


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
    unit grew) is the same kernel -- branches are relative and the encodings stay in the text -- and without the padding up to
    the next kernel's alignment (s_nop 0, s_code_end or elided zeros after the last instruction), which depends on what follows"""
    out = {}
    for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M):
        lines = re.sub(r"// [0-9A-F]+:", "//", m.group(2)).split("\n")
        while lines and PADDING.match(lines[-1]):
            lines.pop()
        out[m.group(1)] = "\n".join(lines)
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


def without_pcrel(body):
    """-> the body with the literals of the s_add_u32 / s_addc_u32 pair directly after an s_getpc_b64 (text and encoding dword)
    replaced by a placeholder.  Only that pair, and only on the registers the s_getpc_b64 wrote: any other literal stays"""
    lines = body.split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"\s*s_getpc_b64 s\[(\d+):(\d+)\]", line)
        if not m:
            continue
        for j, (op, reg) in enumerate((("s_add_u32", m.group(1)), ("s_addc_u32", m.group(2))), 1):
            if i + j >= len(lines):
                break
            lines[i + j], n = re.subn(rf"^(\s*{op} s{reg}, s{reg}, )\S+(\s*// [0-9A-F]{{8}}) [0-9A-F]{{8}}\s*$", r"\1pcrel\2 pcrel",
                                      lines[i + j])
            if not n:
                break
    return "\n".join(lines)


def unit(obj):
    """-> (disassembly, metadata) of an object file, or None for a unit without device code"""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        if co is None:
            return None
        return disassembly(co), metadata(co)


def kernels(units):
    """{unit name: (disassembly, metadata) or None} -> {symbol: (unit name, body, metadata or None)}, and the report lines of every
    symbol that a second unit defines too: only one body per symbol is compared, so such a build is never called identical"""
    out, twice = {}, []
    for name, u in units.items():
        if u is None:
            continue
        asm, meta = u
        for sym, body in functions(asm).items():
            if sym in out:
                twice.append(f"{name}: code  {sym}: defined in {out[sym][0]} too, only that one is compared")
                continue
            out[sym] = (name, body, meta.get(sym))
    return out, twice


def compare(a_units, b_units):
    """-> (report lines, True if anything but constant addresses differs)"""
    (ka, twice_a), (kb, twice_b) = kernels(a_units), kernels(b_units)
    lines = [f"first build: {t}" for t in twice_a] + [f"second build: {t}" for t in twice_b]
    bad = bool(lines)
    n_const = n_moved = 0
    for name in sorted(b_units):
        if b_units[name] is None:
            same = a_units.get(name, None) is None
            lines.append(f"{name}: {'no device code' if same else 'device code in the first build only'}")
            continue
        syms = sorted(s for s, (u, _, _) in kb.items() if u == name)
        n_kern = sum(1 for s in syms if kb[s][2] is not None)
        detail, const, moved = [], [], {}
        for s in syms:
            if s not in ka:
                detail.append(f"    code  {s}: in the second build only")
                continue
            (ua, body_a, meta_a), (_, body_b, meta_b) = ka[s], kb[s]
            if ua != name:
                moved[ua] = moved.get(ua, 0) + 1
            if meta_a != meta_b:
                detail.append(f"    meta  {s}: {meta_a} -> {meta_b}")
            if body_a == body_b:
                continue
            if without_pcrel(body_a) == without_pcrel(body_b):
                const.append(s)
            else:
                detail.append(f"    code  {s}: {len(body_a.splitlines())} -> {len(body_b.splitlines())} instructions")
        n_const += len(const)
        n_moved += sum(moved.values())
        verdict = f"{len(detail)} differ" if detail else "constant address only" if const else "identical"
        origin = "".join(f", {n} moved here from {u}" for u, n in sorted(moved.items()))
        lines.append(f"{name}: {n_kern} kernels, {len(syms)} symbols{origin}: {verdict}")
        lines += detail + [f"    constant address only  {s}" for s in const]
        bad |= bool(detail)
    for s in sorted(set(ka) - set(kb)):
        lines.append(f"{ka[s][0]}: code  {s}: in the first build only")
        bad = True
    total = sum(1 for v in kb.values() if v[2] is not None)
    lines.append(("DIFFERENT" if bad else "IDENTICAL") + f": {len(b_units)} units, {total} kernels, {n_moved} in another unit than before, "
                 f"{n_const} differ in constant addresses only")
    return lines, bad


def build_units(build_dir):
    return {f: unit(os.path.join(build_dir, f)) for f in sorted(os.listdir(build_dir)) if f.endswith(".o")}


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    lines, bad = compare(build_units(argv[1]), build_units(argv[2]))
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
