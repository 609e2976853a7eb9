"""Host branch of rcpf_, sqrtf_ and rsqrt_exact (csrc/frt_math.hpp): still the plain IEEE expression, which is what tests/hostcheck and the
oracle comparison rest on. tools/_build/exact_div_sqrt_host (host-only build of the header, built by build()) evaluates them on a file of
operands; numpy's float32 division and square root (correctly rounded) are the reference. CPU only."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "_build", "exact_div_sqrt_host")


def operands():
    rng = np.random.default_rng(20261019)
    rnd = rng.integers(0, 2 ** 32, size=3_000_000, dtype=np.uint64).astype(np.uint32)      # random bit patterns: every exponent, NaNs, denormals
    near_one = (np.float32(0.25) + rng.random(1_000_000, dtype=np.float32) * np.float32(7.75)).view(np.uint32)
    exps = np.arange(256, dtype=np.uint32) << 23
    mant = np.array([0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF], dtype=np.uint32)
    edge = (exps[:, None] | mant[None, :]).ravel()
    edge = np.concatenate([edge, edge | np.uint32(0x80000000)])
    return np.concatenate([rnd, near_one, edge]).view(np.float32)


def same(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def evaluated(tmp_path_factory):
    assert os.path.exists(TOOL), "tools/_build/exact_div_sqrt_host is not built (python __graft_entry__.py)"
    d = tmp_path_factory.mktemp("exact_div_sqrt")
    x = operands()
    x.tofile(d / "in.f32")
    subprocess.run([TOOL, str(d / "in.f32"), str(d / "out.f32")], check=True, timeout=60)
    y = np.fromfile(d / "out.f32", dtype=np.float32).reshape(3, x.size)
    return x, y


def test_host_rcp_is_ieee_division(evaluated):
    x, y = evaluated
    with np.errstate(all="ignore"):
        want = np.float32(1.0) / x
    bad = ~same(y[0], want)
    assert not bad.any(), x[bad][:8].view(np.uint32)


def test_host_sqrt_is_ieee_sqrt(evaluated):
    x, y = evaluated
    with np.errstate(all="ignore"):
        want = np.sqrt(x)
    bad = ~same(y[1], want)
    assert not bad.any(), x[bad][:8].view(np.uint32)


def test_host_rsqrt_is_division_by_the_square_root(evaluated):
    x, y = evaluated
    with np.errstate(all="ignore"):
        want = np.float32(1.0) / np.sqrt(x)
    bad = ~same(y[2], want)
    assert not bad.any(), x[bad][:8].view(np.uint32)
