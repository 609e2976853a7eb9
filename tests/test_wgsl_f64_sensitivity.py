"""The float64 references must be able to fail: each misreading of the shader text that motivates them (tests/_wgsl_f64.py, `mis`),
applied to the float64 side only, makes the comparison against the oracle fail at the tolerances the comparisons use."""
import numpy as np
import pytest
import _wgsl_f64 as R
import test_wgsl_f64_gbuffer as G
import test_wgsl_f64_post as P
import test_wgsl_f64_restir as T


@pytest.mark.parametrize("mis,scene_name,cam_name", [("m_inv_transposed", "transforms", "static"), ("tbn_transposed", "textured", "static"),
                                                     ("motion_sign", "cornell", "moving"), ("no_y_flip", "cornell", "moving"),
                                                     ("oct_sign", "textured", "static"), ("clamp_to_edge", "textured", "static")])
def test_gbuffer_misreading_is_caught(frt, orc, mis, scene_name, cam_name):
    fs, os_, tex = G.SCENES[scene_name](frt, orc)
    W, H = 128, 72
    cam = G.camera(frt, cam_name, W / H)
    ro = os_.renderer(W, H, 1, True, 8)
    ro.render_phases(cam, 1, 0, H)
    got = G._read_oracle(ro)
    sc = R.scene_arrays(fs)
    _, bad = G.residuals(got, G.reference(frt, scene_name, cam_name, W, H, sc, tex))
    assert not bad, bad                                  # the faithful reading agrees ...
    _, bad = G.residuals(got, R.gbuffer_f64(sc, cam, W, H, tex, mis={mis}))
    assert bad, f"{mis}: the comparison does not notice this misreading"      # ... and the misreading does not
    print(f" {mis}: {bad[0]}")



@pytest.mark.parametrize("mis,W,H,fc", [("history_clamped", 15, 17, 1), ("speed_le", 16, 16, 1)])
def test_post_misreading_is_caught(frt, orc, mis, W, H, fc):
    """history_clamped: off-image history taps read the nearest pixel instead of contributing 0 (post.wgsl:219-222, kept on purpose);
    speed_le: the still / moving switch taken at speed == 0.5 (crafted: exactly half a pixel along x, exact in f32 at W = 16)."""
    _, _, (inp, accum, display) = P._oracle_case(frt, orc, W, H, fc, (0.0, 0.0))
    P.check(inp, accum, display, W, H, fc, (0.0, 0.0))                              # the faithful reading agrees ...
    with pytest.raises(AssertionError):
        P.check(inp, accum, display, W, H, fc, (0.0, 0.0), mis={mis})               # ... and the misreading does not


TEMPORAL_MIS = ["other_reservoirs", "temporal_m20", "ratio_inverted", "ris_le", "normal_0995", "prev_id_rounded"]
SPATIAL_MIS = ["spatial_m16", "ris_le", "no_rescale", "jacobian_no_albedo", "jacobian_clamp_05_2", "offset_rounded", "third_draw_always", "tmax_dist"]
RESTIR_CASE = ("probe", 64, 48, 0)


@pytest.mark.parametrize("mis", TEMPORAL_MIS)
def test_temporal_misreading_is_caught(frt, orc, mis):
    """Each misreading of restir.wgsl:842-917 (tests/_wgsl_f64_restir.py, `mis`) on the float64 side only fails the comparison with the oracle."""
    which, W, H, fc = RESTIR_CASE
    _, _, _, view_pos, mats = T._setup(frt, orc, which, W, H, fc)
    inp, out = T.oracle_temporal(frt, orc, which, W, H, fc)
    T.check_temporal(inp, out, W, H, fc, view_pos, mats)                            # the faithful reading agrees ...
    with pytest.raises(AssertionError, match="pixels differ from float64"):
        T.check_temporal(inp, out, W, H, fc, view_pos, mats, mis={mis})             # ... and the misreading does not


@pytest.mark.parametrize("mis", SPATIAL_MIS)
def test_spatial_misreading_is_caught(frt, orc, mis):
    """The same for restir_spatial.wgsl:857-993."""
    which, W, H, fc = RESTIR_CASE
    fs, _, _, view_pos, mats = T._setup(frt, orc, which, W, H, fc)
    inp, out, raw = T.oracle_spatial(frt, orc, which, W, H, fc)
    T.check_spatial(inp, out, raw, W, H, fc, view_pos, mats, T.tris_of(fs, which))
    with pytest.raises(AssertionError, match="pixels differ from float64"):
        T.check_spatial(inp, out, raw, W, H, fc, view_pos, mats, T.tris_of(fs, which), mis={mis})


SHADE_MIS = [("g1_alpha2", "g1"), ("prob_spec_swapped", "eval_pdf"), ("fresnel_n_dot_v", "eval_bsdf"), ("pdf_g_smith", "eval_pdf"), ("kd_no_metallic", "eval_bsdf"),
             ("glass_ratio_swapped", "sample_bsdf"), ("glass_no_short_circuit", "sample_bsdf"), ("vndf_no_stretch_back", "vndf"), ("sphere_radius_u", "light"),
             ("mis_power", "nee0"), ("nee_tmax_dist", "nee1"), ("nee_pdf_from_offset", "nee0"), ("roulette_ge", "roulette"), ("offset_no_sign", "roulette")]


@pytest.mark.parametrize("mis,op", SHADE_MIS)
def test_shading_misreading_is_caught(orc, mis, op):
    """Each misreading of restir.wgsl:161-603 (tests/_wgsl_f64_shade.py, `mis`) on the float64 side only puts at least one case that the misread
    float64 still decides outside its bound, or off in its draw count, against the oracle."""
    import _shade_probe as S
    inp, _, lights, ref, und = S.prepared(op)
    out = S.run_oracle(orc, op, inp, lights)
    assert not S.failures(S.compare(op, out, ref, und)).any()                      # the faithful reading agrees ...
    bad_ref, bad_und = S.reference(op, inp, lights, mis={mis})
    bad = S.failures(S.compare(op, out, bad_ref, bad_und))
    assert bad.any(), f"{mis}: the comparison does not notice this misreading"   # ... and the misreading does not
    print(f" {mis}: {int(bad.sum())} of {len(inp)} cases of {op}")
