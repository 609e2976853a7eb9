"""The shading arithmetic of trace_path, one call at a time, against its float64 restatement (tests/_wgsl_f64_shade.py, written from restir.wgsl
alone): make_orthonormal_basis, fresnel_schlick, reflectance, ndf_ggx, geometry_schlick_ggx, sample_ggx_vndf, sample_light, eval_pdf, eval_bsdf,
random_unit_vector, sample_bsdf, the NEE block in both variants of its shadow ray and Russian roulette with the ray offset. Crafted and random cases
(tests/_shade_probe.py: cases), a few thousand per operation, run through the oracle's own functions (orc_shade_probe) and through the product's
headers compiled for the host (hc_shade_probe: the probe body of tests/hostcheck/frt_shade_probe.hpp). The end-to-end candidate path is not compared
with float64 here or anywhere: it is chaotic, and stays compared between product and oracle only.

(a) the two f32 builds agree in every output word of every case (two NaNs are equal; nothing is exempt);
(b) every f32 output of a case float64 can decide lies within its derived per-case bound (_wgsl_f64_shade.py: E), and wherever that bound is made of
    at least LONG_CHAIN roundings BY WEIGHT (_shade_probe.py: LONG_CHAIN, where the deviation from a plain count is stated) the oracle uses at most
    ORACLE_SHARE of it; at most MAX_UNDECIDED of any group is undecided, except the groups
    built to be undecided (BUILT_UNDECIDED), which float64 must flag entirely;
(c) the rng word after the call, hence the number of draws taken, equals float64's exactly for every decided case.
The worst shares per operation are kept in profiles/shade_f64.md."""
import numpy as np
import pytest
import _shade_probe as S

BUILDS = ["oracle", "host"]


@pytest.fixture(scope="module")
def outputs(orc, hostcheck):
    out = {}
    for op in S.OPS:
        inp, _, lights, _, _ = S.prepared(op)
        out[op] = {"oracle": S.run_oracle(orc, op, inp, lights), "host": S.run_host(hostcheck, op, inp, lights)}
    return out


def test_record_sizes_agree(orc, hostcheck):
    assert S.sizes_oracle(orc) == S.sizes_expected()
    assert S.sizes_host(hostcheck) == S.sizes_expected()


def test_case_counts():
    total = 0
    for op in S.OPS:
        n = len(S.prepared(op)[0])
        assert n % 64 != 0 and n % 256 != 0, f"{op}: {n} cases leave the tail guard idle"
        total += n
    assert total < 200_000


def test_pcg_unhash_inverts_pcg_hash():
    import _wgsl_f64_shade as R
    x = np.random.default_rng(5).integers(0, 2 ** 32, 100_000, dtype=np.uint64)
    assert (R.pcg_hash(R.pcg_unhash(x)) == x).all() and (R.pcg_unhash(R.pcg_hash(x)) == x).all()


@pytest.mark.parametrize("op", S.OPS)
def test_host_build_equals_oracle_bit_for_bit(outputs, op):
    diff = S.words_differ(outputs[op]["oracle"], outputs[op]["host"])
    i = np.nonzero(diff)[0]
    assert not len(i), f"{op}: {len(i)} cases differ, first {i[0]}: {S.prepared(op)[0][i[0]]} -> {outputs[op]['oracle'][i[0]]} vs {outputs[op]['host'][i[0]]}"


@pytest.mark.parametrize("op", S.OPS)
def test_undecided_share_per_group(op):
    _, groups, _, _, und = S.prepared(op)
    for name, ix in groups.items():
        share = float(und[ix].mean())
        print(f" {op}/{name}: {len(ix)} cases, {share:.3f} undecided")
        if (op, name) in S.BUILT_UNDECIDED:
            assert share == 1.0, f"{op}/{name} is built to be undecided, float64 decides {int((~und[ix]).sum())} of its cases"
        else:
            assert share <= S.MAX_UNDECIDED, f"{op}/{name}: float64 leaves {share:.3f} of the cases undecided"


def test_every_named_built_undecided_group_exists():
    for op, name in S.BUILT_UNDECIDED:
        assert name in S.prepared(op)[1]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("op", S.OPS)
def test_outputs_within_float64_bounds(outputs, op, build):
    inp, groups, _, ref, und = S.prepared(op)
    c = S.compare(op, outputs[op][build], ref, und)
    print(f" {op} [{build}]: worst share of bound {c['share'].max():.3f}, over its {int(c['n_long'].sum())} long outputs {c['long_share'].max():.3f}, {int((~und).sum())} decided cases")
    for name, ix in groups.items():
        print(f"   {name}: {c['share'][ix].max():.3f}")
    bad = np.nonzero((c["share"] > 1.0) | c["int_bad"])[0]
    assert not len(bad), f"{op}: {len(bad)} decided cases outside their bound, first {bad[0]}: {inp[bad[0]]} -> {outputs[op][build][bad[0]]} (share {c['share'][bad[0]]:.3f})"
    if build == "oracle":
        assert c["long_share"].max() <= S.ORACLE_SHARE, "the f32 reading uses more than half of a long chain's derived bound: the derivation (or the reading) is off"


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("op", [op for op in S.OPS if "rng" in S.OUT[op].names])
def test_draw_accounting(outputs, op, build):
    inp, _, _, ref, und = S.prepared(op)
    c = S.compare(op, outputs[op][build], ref, und)
    bad = np.nonzero(c["rng_bad"])[0]
    assert not len(bad), f"{op}: rng after differs from float64's in {len(bad)} decided cases, first {bad[0]}: {inp[bad[0]]}"


def test_crafted_branches_are_reached(outputs):
    """The cases the generators are built for do what they are built for, on the oracle."""
    o = outputs["sample_bsdf"]["oracle"]; g = S.prepared("sample_bsdf")[1]
    zero_wi = (o["wi"][g["glass_k_negative"]] == 0).all(1)
    print(f" glass_k_negative: {int(zero_wi.sum())} of {len(zero_wi)} cases refract into the zero vector")
    assert zero_wi.any(), "no case of glass_k_negative reaches refract()'s zero vector after the test of :318 said refract"
    g_spec = S.prepared("sample_bsdf")[1]["specular_glossy"]
    assert len(g_spec) >= 1000 and not S.prepared("sample_bsdf")[4][g_spec].any()
    assert (o["weight"][g["ndv_negative"]] == 0).all() and (o["pdf"][g["ndv_negative"]] == 0).all()
    assert (o["weight"][g["grazing_below_surface"]] == 0).all(1).any()
    for op in ("nee0", "nee1"):
        o = outputs[op]["oracle"]; g = S.prepared(op)[1]
        assert (o["nee"][g["draw_is_one"]] == 0).all() and (o["nee"][g["no_lights"]] == 0).all()
        assert (o["nee"][g["light_behind_surface"]] == 1).all()
        assert (o["nee"][g["tiny_dist_early_out"]] == (2 if op == "nee0" else 3)).all()
        assert set(np.unique(o["nee"][g["bulk"]])) >= {1, 2}
    o = outputs["roulette"]["oracle"]; g = S.prepared("roulette")[1]
    assert set(o["survived"][g["draw_sides"]]) == {0, 1} and (o["survived"][g["draw_equals_survival"]] == 1).all()
