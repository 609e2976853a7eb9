"""The device leg of tests/test_wgsl_f64_shade.py: the same cases through tools/_build/shade_probe — the product's headers (csrc/frt_path.hpp and what
it includes, unchanged) compiled for gfx950 under the product's device flags, one thread per case. The probe is not the product's kernel. The numeric
contract promises that this arithmetic does not depend on which kernel it is inlined into, and the every-buffer parity tests tie the production
kernels to the oracle; this file ties the same headers on the device — rcpf_, neg_rcpf_, sqrtf_, rsqrt_exact included — to the oracle and to the
host build bit for bit on every case, and to float64 within the derived bounds. It claims no more than that."""
import tempfile

import numpy as np
import pytest
import _shade_probe as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def outputs(orc, hostcheck):
    import os
    assert os.path.exists(S.TOOL), "tools/_build/shade_probe is not built (python __graft_entry__.py)"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for op in S.OPS:                      # one after another; the first failure or timeout raises and starts nothing further
            inp, _, lights, _, _ = S.prepared(op)
            out[op] = {"device": S.run_device(op, inp, lights, tmp, timeout=60)}
    for op in S.OPS:
        inp, _, lights, _, _ = S.prepared(op)
        out[op]["oracle"] = S.run_oracle(orc, op, inp, lights)
        out[op]["host"] = S.run_host(hostcheck, op, inp, lights)
    return out


@pytest.mark.parametrize("other", ["oracle", "host"])
@pytest.mark.parametrize("op", S.OPS)
def test_device_equals_cpu_builds_bit_for_bit(outputs, op, other):
    diff = S.words_differ(outputs[op]["device"], outputs[op][other])
    i = np.nonzero(diff)[0]
    assert not len(i), f"{op}: {len(i)} cases differ from the {other}, first {i[0]}: {S.prepared(op)[0][i[0]]} -> {outputs[op]['device'][i[0]]} vs {outputs[op][other][i[0]]}"


@pytest.mark.parametrize("op", S.OPS)
def test_device_outputs_within_float64_bounds(outputs, op):
    inp, groups, _, ref, und = S.prepared(op)
    c = S.compare(op, outputs[op]["device"], ref, und)
    print(f" {op} [device]: worst share of bound {c['share'].max():.3f}, over its {int(c['n_long'].sum())} long outputs {c['long_share'].max():.3f}, {int((~und).sum())} decided cases")
    bad = np.nonzero(S.failures(c))[0]
    assert not len(bad), f"{op}: {len(bad)} decided cases outside their bound or off in their draws, first {bad[0]}: {inp[bad[0]]} -> {outputs[op]['device'][bad[0]]}"
