"""The device forms of 1 / x, sqrt(x) and 1 / sqrt(x) (csrc/frt_math.hpp: rcpf_, sqrtf_, rsqrt_exact, neg_rcpf_) against the compiler's correctly
rounded `1.0f / x` and `__builtin_sqrtf(x)`: all 2^32 bit patterns of x, both sides in one kernel under the product's flags
(tools/exact_div_sqrt_check.hip, built by build()). The tool runs once; every test reads its one JSON line."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "_build", "exact_div_sqrt_check")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def result():
    assert os.path.exists(TOOL), "tools/_build/exact_div_sqrt_check is not built (python __graft_entry__.py)"
    p = subprocess.run([TOOL], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().split("\n")[-1])
    for name, r in res.items():
        print(f"{name}: {r['mismatches']} mismatches of {r['patterns']} patterns, {r['fast_path']} on the fast path, first {r['first']}")
    return res


@pytest.mark.parametrize("form", ["rcp", "sqrt", "rsqrt", "neg_rcp"])
def test_form_equals_the_compilers_for_every_bit_pattern(result, form):
    r = result[form]
    assert r["patterns"] == 2 ** 32
    assert r["mismatches"] == 0, f"{form}: {r['mismatches']} operands differ from the compiler's expansion, e.g. {r['first']}"
    assert r["first"] == []


def test_the_fast_paths_are_what_was_compared(result):
    """A form that sent every operand to its fallback would pass trivially. rcp: both signs of [2^-126, 2^126); sqrt and rsqrt:
    [2^-96, 2^126) (frt_math.hpp: rcp_fast_range, sqrt_fast_range)."""
    assert result["rcp"]["fast_path"] == 2 * 252 * 2 ** 23
    assert result["neg_rcp"]["fast_path"] == 2 * 252 * 2 ** 23
    assert result["sqrt"]["fast_path"] == 222 * 2 ** 23
    assert result["rsqrt"]["fast_path"] == 222 * 2 ** 23
