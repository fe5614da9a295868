"""The route arithmetic of the Gaussian and the gradient (csrc/gauss_route.hpp) on the CPU: tools/gauss_route_check.cpp walks
every radius 0 ... 260 under every switch setting through the launchers' decisions and asserts that each kernel they pick
is one the units build, that each kernel built is picked by some call, and that no LDS size exceeds 160 KB.  The program is
compiled with the host sanitizers (their runtimes linked statically) and run on its own; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_rules_pick_exactly_the_kernels_that_are_built(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path / "gauss_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "topo_descriptors_amd", "csrc"),
                    os.path.join(ROOT, "tools", "gauss_route_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "all ok" in out.stdout
