"""The host side of libplipmi.so under AddressSanitizer + UBSan, on the CPU: tests/native/host_checks.hip is a
stand-alone program over the library's host translation units -- config validation, every export's early returns, the hook
setters, the pass arithmetic, shape resolution and the two-pass slab carving (csrc/handle_host.h).  The host units and the
program are compiled with the sanitizers; the kernel objects are the library's own, as built.  Nothing here touches a GPU."""
import concurrent.futures as cf
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_UNITS = ("engine.hip", "towers.hip", "heads.hip", "test_entries.hip")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
            "-Xarch_host", "-fno-omit-frame-pointer", "-g"]


def test_host_code_is_clean_under_address_and_ub_sanitizers(tmp_path):
    from plip_amd import build as B
    try:
        hipcc = B._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    B.build(verbose=False)                      # the kernel objects the program links against
    assert set(HOST_UNITS) <= set(B.SOURCES)
    kernel_objs = [os.path.join(B.BUILD, s.replace(".hip", ".o")) for s in B.SOURCES if s not in HOST_UNITS]
    units = [os.path.join(B.CSRC, u) for u in HOST_UNITS] + [os.path.join(ROOT, "tests", "native", "host_checks.hip")]

    def compile_one(src):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        r = subprocess.run([hipcc, *B.FLAGS, *SANITIZE, "-I", B.CSRC, "-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        return obj

    with cf.ThreadPoolExecutor(max_workers=len(units)) as ex:
        objs = list(ex.map(compile_one, units))
    exe = str(tmp_path / "host_checks")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", *SANITIZE[:2], *objs, *kernel_objs, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # no device for the program, wherever it runs: plipmi_create's last answer is then PLIPMI_ERR_NODEVICE
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "host checks passed" in r.stdout
    for report in ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED"):
        assert report not in out, out[-6000:]
