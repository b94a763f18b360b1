"""The host paths of capes (the builder with and without a cape, the cape <-> texel maps, the refusals, the caped view table of
every skin kind) under AddressSanitizer + UBSan: a stand-alone program with its own main, tests/cpp/asan_cape_host.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minecraftskin_raytracer_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cape_host_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "asan_cape_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{CSRC}",
                           os.path.join(ROOT, "tests", "cpp", "asan_cape_host.cpp"), os.path.join(CSRC, "flatten.cpp"),
                           os.path.join(CSRC, "scene_builder.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "asan cape driver: 0 problem(s)" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
