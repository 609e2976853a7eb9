"""Morph targets from plain C: tests/cabi/frt_cabi_morph.c includes include/frt.h, links libfrt.so and nothing else, binds targets, morphs, morphs and
poses, and reads the triangles back. The scene half runs anywhere; with the argument "gpu" it repeats the calls on a renderer and compares the replica."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cabi", "frt_cabi_morph.c")
OUT = os.path.join(ROOT, "tests", "cabi", "_build", "frt_cabi_morph")
LIBDIR = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "lib")


def _build(frt):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), SRC, "-L", LIBDIR, "-lfrt",
                    f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", OUT], check=True)


def test_c_host_binds_and_morphs(frt):
    _build(frt)
    p = subprocess.run([OUT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("morph ok")


@pytest.mark.gpu
def test_c_host_morphs_a_renderer(frt):
    if frt.lib().frt_device_count() < 1:
        pytest.fail("no HIP device")
    _build(frt)
    p = subprocess.run([OUT, "gpu"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("morph ok (gpu)")
