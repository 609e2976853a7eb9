"""Records, cases, runners and the comparison of the shading probes (tests/test_wgsl_f64_shade.py, _gpu.py, test_wgsl_f64_sensitivity.py).
IN / OUT are THE definition of the record layouts (little-endian, every field a 4-byte word, no padding); the C++ structs of
tests/hostcheck/frt_shade_probe.hpp (device and host build) and oracle/orc_render.cpp (oracle) restate them and report their sizes."""
import ctypes as C
import os
import subprocess

import numpy as np

import _wgsl_f64_shade as R

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "_build", "shade_probe")
OPS = ["basis", "fresnel", "reflectance", "ndf", "g1", "vndf", "light", "eval_pdf", "eval_bsdf", "unit_vector", "sample_bsdf", "nee0", "nee1", "roulette"]
NUM_TABLE_LIGHTS = 100
# The long-chain rule. The issue words it as a count: outputs whose chain counts at least LONG_CHAIN roundings use at most ORACLE_SHARE of their bound
# on the oracle. tests/test_wgsl_f64_restir.py applies that as bound >= LONG_CHAIN * EPS * |value|, which is the count only where the conditioning
# is 1 (sums of non-negative terms). Here it is not: a cancelling sum (a light position near 0, refract's difference) has a bound of many EPS * |value|
# made of two or three roundings, and a chain of a dozen operations (reflectance, g1) is often dominated by its last rounding, which reaches its worst
# case for real. So this file DEVIATES from the issue's wording and counts by weight: an output is long when its bound is at least LONG_CHAIN times
# the largest single rounding's contribution to it (_wgsl_f64_shade.py: E.n, carried through the same conditioning as the bound; through a product
# as a sum, since x * x carries x's rounding twice). Outputs with an exact bound of 0 are not long. By plain operation count reflectance (about 12,
# share 0.65) and g1 (about 10, share 0.51) would exceed ORACLE_SHARE; their bounds are not widened, they are only not held to the half.
LONG_CHAIN = 8
ORACLE_SHARE = 0.5
MAX_UNDECIDED = 0.02

V3 = ("<f4", (3,))
LIGHT = np.dtype([("position", *V3), ("type", "<u4"), ("u", *V3), ("area", "<f4"), ("v", *V3), ("pad", "<u4"), ("emission", "<f4", (4,))])
_MAT = [("roughness", "<f4"), ("metallic", "<f4"), ("transmission", "<f4"), ("ior", "<f4")]
_EVAL = [("n", *V3), ("wi", *V3), ("wo", *V3)] + _MAT + [("base", *V3)]
_NEE_IN = [("num_lights", "<u4"), ("pos", *V3), ("ffn", *V3), ("wo", *V3)] + _MAT + [("base", *V3), ("visible", "<u4"), ("rng", "<u4")]
_NEE_OUT = [("nee", "<u4"), ("want", "<u4"), ("o", *V3), ("d", *V3), ("tmin", "<f4"), ("tmax", "<f4"), ("direct", *V3), ("rng", "<u4")]
IN = {
    "basis": [("n", *V3)], "fresnel": [("f0", *V3), ("v_dot_h", "<f4")], "reflectance": [("cosine", "<f4"), ("ref_idx", "<f4")],
    "ndf": [("n_dot_h", "<f4"), ("roughness", "<f4")], "g1": [("n_dot_v", "<f4"), ("roughness", "<f4")],
    "vndf": [("wo", *V3), ("roughness", "<f4"), ("u", "<f4", (2,))], "light": [("light", LIGHT), ("rng", "<u4")],
    "eval_pdf": _EVAL, "eval_bsdf": _EVAL, "unit_vector": [("rng", "<u4")],
    "sample_bsdf": [("wo", *V3), ("ffn", *V3), ("front", "<u4")] + _MAT + [("base", *V3), ("rng", "<u4")],
    "nee0": _NEE_IN, "nee1": _NEE_IN,
    "roulette": [("depth", "<u4"), ("throughput", *V3), ("ffn", *V3), ("next_dir", *V3), ("pos", *V3), ("rng", "<u4")],
}
OUT = {
    "basis": [("tangent", *V3), ("bitangent", *V3)], "fresnel": [("f", *V3)], "reflectance": [("r", "<f4")], "ndf": [("d", "<f4")], "g1": [("g", "<f4")],
    "vndf": [("wm", *V3)], "light": [("pos", *V3), ("normal", *V3), ("pdf", "<f4"), ("emission", "<f4", (4,)), ("rng", "<u4")],
    "eval_pdf": [("pdf", "<f4")], "eval_bsdf": [("f", *V3)], "unit_vector": [("v", *V3), ("rng", "<u4")],
    "sample_bsdf": [("wi", *V3), ("pdf", "<f4"), ("weight", *V3), ("rng", "<u4")], "nee0": _NEE_OUT, "nee1": _NEE_OUT,
    "roulette": [("survived", "<u4"), ("throughput", *V3), ("origin", *V3), ("rng", "<u4")],
}
IN = {k: np.dtype(v) for k, v in IN.items()}
OUT = {k: np.dtype(v) for k, v in OUT.items()}
# groups float64 cannot decide by construction: asserted to BE flagged instead of being held to MAX_UNDECIDED
BUILT_UNDECIDED = {("ndf", "ndh_1_rough_0_001"), ("eval_pdf", "ndh_1_rough_0_001"), ("eval_bsdf", "ndh_1_rough_0_001"), ("sample_bsdf", "glass_k_negative"),
                   ("g1", "zero_over_zero"), ("eval_pdf", "ndv_one_ulp"), ("vndf", "u_x1_corners"), ("light", "degenerate_quad"), ("sample_bsdf", "rough0_specular"), ("sample_bsdf", "specular_rough_005")}


# ------------------------------------------------------------------------------------------------ runners
def sizes_expected():
    return [s for op in OPS for s in (IN[op].itemsize, OUT[op].itemsize)]


def sizes_oracle(orc):
    s = (C.c_uint32 * 28)(); orc.L.orc_shade_probe_sizes(s); return list(s)


def sizes_host(hc):
    s = (C.c_uint32 * 28)(); hc.L.hc_shade_probe_sizes(s); return list(s)


def run_oracle(orc, op, inp, lights):
    out = np.zeros(len(inp), OUT[op])
    inp = np.ascontiguousarray(inp); lights = np.ascontiguousarray(lights)
    assert orc.L.orc_shade_probe(OPS.index(op), lights.ctypes.data, len(lights), inp.ctypes.data, out.ctypes.data, len(inp)) == 0
    return out


def run_host(hc, op, inp, lights):
    out = np.zeros(len(inp), OUT[op])
    inp = np.ascontiguousarray(inp); lights = np.ascontiguousarray(lights)
    assert len(lights) == NUM_TABLE_LIGHTS
    assert hc.L.hc_shade_probe(OPS.index(op), lights.ctypes.data, inp.ctypes.data, out.ctypes.data, len(inp)) == 0
    return out


def run_device(op, inp, lights, tmpdir, timeout=60):
    """One invocation of tools/_build/shade_probe. Raises on a non-zero exit status or a timeout."""
    fin, fout = os.path.join(tmpdir, op + ".in"), os.path.join(tmpdir, op + ".out")
    with open(fin, "wb") as f:
        if op in ("nee0", "nee1"):
            assert len(lights) == NUM_TABLE_LIGHTS
            f.write(np.ascontiguousarray(lights).tobytes())
        f.write(np.ascontiguousarray(inp).tobytes())
    p = subprocess.run([TOOL, op, fin, fout], capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"shade_probe {op}: exit status {p.returncode}: {p.stderr[-2000:]}")
    out = np.fromfile(fout, OUT[op])
    assert len(out) == len(inp)
    return out


def words_differ(a, b):
    """Per record: some output word differs. Two NaNs are equal whatever their payload; +0 and -0 are different words."""
    wa, wb = a.view("<u4").reshape(len(a), -1), b.view("<u4").reshape(len(b), -1)
    fa, fb = wa.view("<f4"), wb.view("<f4")
    isf = np.array([k for name in a.dtype.names for k in [a.dtype[name].base.kind == "f"] * int(np.prod(a.dtype[name].shape or (1,)))])
    nan_both = np.isnan(fa) & np.isnan(fb) & isf[None, :]
    return ((wa != wb) & ~nan_both).any(1)


# ------------------------------------------------------------------------------------------------ float64 side
def _mat(inp):
    return {k: inp[k] for k in ("roughness", "metallic", "transmission", "ior")}


def reference(op, inp, lights, mis=()):
    """-> (dict output field -> E | tuple of E | exact integer array, undecided flag per case)."""
    n = len(inp)
    U = R.Und(n)
    E, vec = R.E, R.vec
    live = np.ones(n, bool)
    if op == "basis":
        t, b = R.make_orthonormal_basis(vec(inp["n"]), U, live); o = {"tangent": t, "bitangent": b}
    elif op == "fresnel":
        o = {"f": R.fresnel_schlick(vec(inp["f0"]), E(inp["v_dot_h"]))}
    elif op == "reflectance":
        o = {"r": R.reflectance(E(inp["cosine"]), E(inp["ref_idx"]))}
    elif op == "ndf":
        o = {"d": R.ndf_ggx(E(inp["n_dot_h"]), E(inp["roughness"]))}
    elif op == "g1":
        o = {"g": R.geometry_schlick_ggx(E(inp["n_dot_v"]), E(inp["roughness"]), mis)}
    elif op == "vndf":
        o = {"wm": R.sample_ggx_vndf(vec(inp["wo"]), E(inp["roughness"]), inp["u"][:, 0], inp["u"][:, 1], U, live, mis)}
    elif op == "light":
        rng, pos, nrm, pdf, em = R.sample_light(inp["light"], inp["rng"], U, live, mis)
        o = {"pos": pos, "normal": nrm, "pdf": pdf, "emission": tuple(E(em[:, k]) for k in range(4)), "rng": rng}
    elif op == "eval_pdf":
        o = {"pdf": R.eval_pdf(vec(inp["n"]), vec(inp["wi"]), vec(inp["wo"]), _mat(inp), vec(inp["base"]), U, live, mis)}
    elif op == "eval_bsdf":
        o = {"f": R.eval_bsdf(vec(inp["n"]), vec(inp["wi"]), vec(inp["wo"]), _mat(inp), vec(inp["base"]), U, live, mis)}
    elif op == "unit_vector":
        rng, v = R.random_unit_vector(inp["rng"]); o = {"v": v, "rng": rng}
    elif op == "sample_bsdf":
        rng, wi, pdf, w = R.sample_bsdf(vec(inp["wo"]), vec(inp["ffn"]), inp["front"] != 0, _mat(inp), vec(inp["base"]), inp["rng"], U, mis)
        o = {"wi": wi, "pdf": pdf, "weight": w, "rng": rng}
    elif op in ("nee0", "nee1"):
        o = R.nee(int(op[-1]), lights, inp["num_lights"], vec(inp["pos"]), vec(inp["ffn"]), vec(inp["wo"]), _mat(inp), vec(inp["base"]), inp["visible"] != 0,
                  inp["rng"], U, mis)
    elif op == "roulette":
        o = R.roulette(inp["depth"], vec(inp["throughput"]), vec(inp["ffn"]), vec(inp["next_dir"]), vec(inp["pos"]), inp["rng"], U, mis)
    else:
        raise KeyError(op)
    und = U.f.copy()
    with np.errstate(all="ignore"):
        for k, val in o.items():
            if isinstance(val, np.ndarray):
                continue
            comps = val if isinstance(val, tuple) else (val,)
            scale = np.max([np.abs(c.v) for c in comps], axis=0)
            for c in comps:
                und |= ~np.isfinite(c.v) | ~np.isfinite(c.e) | (c.e > R.REL_LIMIT * scale)
    return o, und


def compare(op, out, ref, und):
    """-> dict: share (worst |f32 - float64| / bound over the float outputs, per case; inf where an exact value differs), long_share (the same over outputs
    that are long by the rule at LONG_CHAIN above), n_long (how many outputs of the case are long), int_bad (an integer output other than rng differs), rng_bad. Undecided cases report zeros."""
    n = len(out)
    share, long_share, n_long = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    int_bad, rng_bad = np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for k, val in ref.items():
            got = out[k]
            if isinstance(val, np.ndarray):
                bad = got.astype(np.int64) != np.asarray(val).astype(np.int64)
                if k == "rng":
                    rng_bad |= bad
                else:
                    int_bad |= bad
                continue
            comps = val if isinstance(val, tuple) else (val,)
            for j, c in enumerate(comps):
                g = (got[:, j] if got.ndim == 2 else got).astype(np.float64)
                d = np.abs(g - c.v)
                s = np.where(c.e > 0, d / c.e, np.where(d == 0, 0.0, np.inf))
                s = np.where(np.isnan(s), np.inf, s)
                share = np.maximum(share, s)
                is_long = (c.e > 0) & (c.e >= LONG_CHAIN * c.n)
                n_long += is_long
                long_share = np.maximum(long_share, np.where(is_long, s, 0.0))
    z = lambda a: np.where(und, 0, a)
    return {"share": z(share), "long_share": z(long_share), "n_long": z(n_long), "int_bad": int_bad & ~und, "rng_bad": rng_bad & ~und}


def failures(cmp_):
    return (cmp_["share"] > 1.0) | cmp_["int_bad"] | cmp_["rng_bad"]


# ------------------------------------------------------------------------------------------------ cases
ROUGH = [0.0, 0.01, 0.049, 0.05, 0.2, 0.5, 1.0]
METAL = [0.0, 0.5, 1.0]
COLOURS = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.9, 0.6, 0.1)]
_TOP = 0xFFFFFFFF


def _unit(g, n):
    v = g.normal(size=(n, 3)); return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _hemi(g, nrm, zmin=0.02):
    """Unit vectors with dot(nrm, .) >= about zmin."""
    v = _unit(g, len(nrm)).astype(np.float64)
    d = (v * nrm).sum(1, keepdims=True)
    v = v - 2 * np.minimum(d, 0) * nrm
    v = v + zmin * nrm
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _seed_for_draw(value):
    """The rng word whose first rand() is the f32 nearest to `value` from below (value in [0, 1])."""
    w = np.clip(np.floor(np.asarray(value, np.float64) * 2.0 ** 32), 0, _TOP).astype(np.uint64)
    return R.pcg_unhash(w).astype(np.uint32)


class Cases:
    def __init__(self, op):
        self.op, self.parts, self.groups = op, [], {}

    def add(self, name, **fields):
        n = max(np.shape(v)[0] for v in fields.values() if np.ndim(v) > 0 and not isinstance(v, tuple))
        a = np.zeros(n, IN[self.op])
        for k, v in fields.items():
            a[k] = v
        if self.op in ("eval_pdf", "eval_bsdf", "sample_bsdf", "nee0", "nee1") and "ior" not in fields:
            a["ior"] = 1.5
        start = sum(len(p) for p in self.parts)
        self.parts.append(a)
        self.groups[name] = np.arange(start, start + n)

    def done(self):
        inp = np.concatenate(self.parts)
        while len(inp) % 64 == 0:                       # the tail guard must run: never a whole number of waves or blocks
            inp = np.concatenate([inp, inp[:1]])
            first = next(iter(self.groups)); self.groups[first] = np.append(self.groups[first], len(inp) - 1)
        return inp, self.groups


def _grid(*lists):
    m = np.meshgrid(*[np.arange(len(l)) for l in lists], indexing="ij")
    return [np.asarray(l)[i.ravel()] for l, i in zip(lists, m)]


def light_table():
    g = np.random.default_rng(77)
    t = np.zeros(NUM_TABLE_LIGHTS, LIGHT)
    t["position"] = g.uniform(-0.5, 0.5, (100, 3)); t["type"] = np.arange(100) % 2
    t["u"] = g.uniform(-0.3, 0.3, (100, 3)); t["v"] = g.uniform(-0.3, 0.3, (100, 3))
    t["v"][:, 0] = np.abs(t["v"][:, 0]) + 0.05
    for k in ("position", "u", "v"):                   # lights 0 - 2 near the origin: the small-distance nee cases sit 5e-5 from a sampled point
        t[k][:3] *= f32(0.1)
    t["area"] = g.uniform(0.05, 2.0, 100); t["emission"] = g.uniform(0.1, 1.0, (100, 4)); t["emission"][:, 3] = g.uniform(1, 20, 100)
    return t


def _materials(g, n, rough_min=0.0):
    r = g.choice(ROUGH, n); r = np.where(g.random(n) < 0.5, g.uniform(rough_min, 1, n), np.maximum(r, rough_min))
    return dict(roughness=r, metallic=np.where(g.random(n) < 0.5, g.choice(METAL, n), g.random(n)), base=g.random((n, 3)))


def cases(op, lights=None):
    g = np.random.default_rng(1000 + OPS.index(op))
    c = Cases(op)
    below1 = np.nextafter(f32(1), f32(0))
    if op == "basis":
        c.add("bulk", n=_unit(g, 3001))
        t = np.linspace(0.1, 6.0, 7)
        nz = []
        for z in (0.0, -0.0):
            nz += [(np.cos(a), np.sin(a), z) for a in t]
        up = np.nextafter(f32(-1), f32(0)); s = np.sqrt(1 - float(up) ** 2)
        nz += [(0, 0, -1), (0, 0, 1), (s, 0, up), (0, s, up), (s * 0.6, s * 0.8, up)]
        c.add("nz_edges", n=np.array(nz, f32))
        c.add("axes", n=np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], f32))
    elif op == "fresnel":
        c.add("bulk", f0=g.random((3001, 3)), v_dot_h=g.random(3001))
        col, v = _grid(np.arange(len(COLOURS)), [0.0, 1.0, -0.5, 1.5, np.nan, float(below1), 1e-8])
        c.add("edges", f0=np.array(COLOURS, f32)[col], v_dot_h=v)
    elif op == "reflectance":
        c.add("bulk", cosine=g.random(3001), ref_idx=g.uniform(0.4, 2.5, 3001))
        a, b = _grid([0.0, 1.0, float(below1), 1e-8, 0.5], [1.0, 1 / 1.5, 1.5, 1.33, 2.4])
        c.add("edges", cosine=a, ref_idx=b)
    elif op == "ndf":
        c.add("bulk", n_dot_h=g.random(3001), roughness=np.maximum(_materials(g, 3001)["roughness"], 0.0))
        a, b = _grid([1.0, float(below1)], [0.2, 0.5, 1.0])
        c.add("ndh_at_1", n_dot_h=a, roughness=b)
        # d = n_dot_h^2 (a2 - 1) + 1 cancels to about a2 <= 6e-6 with an error of 3 roundings of 1: roughness 0 (0 / 0), 0.01 (a2 - 1 rounds to -1: D = inf)
        # and, by the derived bound, 0.049 and 0.05 as well
        a, b = _grid([1.0, float(below1)], [0.01, 0.049, 0.05])
        c.add("ndh_1_rough_0_001", n_dot_h=np.append(a, [1.0, below1]), roughness=np.append(b, [0.0, 0.0]))
        a, b = _grid([0.0, 1e-4, 0.5, 0.999], ROUGH)
        c.add("roughness_set", n_dot_h=a, roughness=b)
    elif op == "g1":
        c.add("bulk", n_dot_v=g.random(3001), roughness=_materials(g, 3001)["roughness"])
        a, b = _grid([1e-15, 1e-6, 1e-3, 0.5, float(below1), 1.0], ROUGH)
        c.add("edges", n_dot_v=a, roughness=b)
        c.add("ndv_0", n_dot_v=np.zeros(6, f32), roughness=np.array(ROUGH[1:], f32))
        c.add("zero_over_zero", n_dot_v=np.zeros(1, f32), roughness=np.zeros(1, f32))
    elif op == "vndf":
        z = np.array([[0, 0, 1]], np.float64)
        n = 3001
        c.add("bulk", wo=_hemi(g, np.repeat(z, n, 0)), roughness=np.maximum(_materials(g, n)["roughness"], 0.01), u=g.uniform(0.001, 0.999, (n, 2)))
        r, ux, uy = _grid(ROUGH[1:], [0.3, 0.9], [0.1, 0.6])
        c.add("normal_incidence", wo=np.tile(np.array([0, 0, 1], f32), (len(r), 1)), roughness=r, u=np.stack([ux, uy], 1))
        n = 200
        w = _hemi(g, np.repeat(z, n, 0), 0.0).astype(np.float64); w[:, 2] = g.uniform(1e-4, 1e-2, n); w /= np.linalg.norm(w, axis=1, keepdims=True)
        c.add("grazing", wo=w, roughness=g.choice(ROUGH[2:], n), u=g.uniform(0.01, 0.99, (n, 2)))
        r, uy = _grid(ROUGH[1:], [0.0, 1.0, 0.3])
        c.add("u_x0", wo=_hemi(g, np.repeat(z, len(r), 0)), roughness=r, u=np.stack([np.zeros(len(r)), uy], 1))
        r, uy = _grid(ROUGH[2:], [0.0, 1.0])
        c.add("u_x1_corners", wo=_hemi(g, np.repeat(z, len(r), 0)), roughness=r, u=np.stack([np.ones(len(r)), uy], 1))
        n = 200                                        # r = 1: t1^2 + t2l^2 is 1 up to rounding, so the max(0, .) arm is taken by about half
        uy = np.concatenate([g.uniform(0.05, 0.45, n // 2), g.uniform(0.55, 0.95, n // 2)])
        c.add("u_x1", wo=_hemi(g, np.repeat(z, n, 0), 0.2), roughness=g.choice([0.5, 1.0], n), u=np.stack([np.ones(n), uy], 1))
    elif op == "light":
        t = light_table()
        n = 3001
        c.add("bulk", light=t[g.integers(0, 100, n)], rng=g.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
        seeds = np.concatenate([R.pcg_unhash([0, _TOP]), R.pcg_unhash(R.pcg_unhash([0, _TOP]))]).astype(np.uint32)      # r1 in {0, 1}; r2 in {0, 1}
        c.add("r_edges", light=np.repeat(t[:2], 4), rng=np.tile(seeds, 2))
        a = t[:4].copy(); a["area"] = [1e-30, 1e30, 1e-30, 1e30]
        c.add("area", light=np.tile(a, 5), rng=g.integers(0, 2 ** 32, 20, dtype=np.uint64).astype(np.uint32))
        d = t[[0, 2, 4]].copy(); d["v"] = d["u"] * f32(2.0)
        c.add("degenerate_quad", light=d, rng=np.array([1, 2, 3], np.uint32))
    elif op in ("eval_pdf", "eval_bsdf"):
        n = 3001
        nr = _unit(g, n); m = _materials(g, n)
        c.add("bulk", n=nr, wi=_hemi(g, nr.astype(np.float64)), wo=_hemi(g, nr.astype(np.float64)), transmission=0.0, **m)
        r, mt, col = _grid(ROUGH, METAL, np.arange(len(COLOURS)))
        k = len(r); nr = _unit(g, k)
        c.add("materials", n=nr, wi=_hemi(g, nr.astype(np.float64), 0.1), wo=_hemi(g, nr.astype(np.float64), 0.1), roughness=r, metallic=mt,
              base=np.array(COLOURS, f32)[col], transmission=0.0)
        # prob_spec at both clamps: white metal (lum_diff = 0: 0.999) and black metal seen along the normal (F = 0: 0.001)
        zz = np.tile(np.array([0, 0, 1], f32), (4, 1))
        c.add("prob_spec_clamps", n=zz, wi=_hemi(g, zz.astype(np.float64), 0.3), wo=np.array([(0.6, 0, 0.8), (0, 0.6, 0.8), (0, 0, 1), (0, 0, 1)], f32),
              roughness=0.5, metallic=1.0, base=np.array([(1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0)], f32), transmission=0.0)
        tiny = f32(1.4e-45)
        zs = [0.0, -0.0, tiny, -tiny, 1e-6, 1e-3, -1e-3]
        wi = np.array([(np.sqrt(max(0, 1 - float(z) ** 2)), 0, z) for z in zs], f32)
        a, b = _grid(np.arange(len(zs)), np.arange(len(zs)))
        rr = np.resize(np.array([0.05, 0.2, 0.5, 1.0], f32), len(a))
        one_ulp = (b == 2) & np.isin(a, [2, 4, 5])           # n_dot_v one ulp above 0 under a positive n_dot_l: G1(v) and pdf_spec are denormal quotients
        keep = ~one_ulp
        zn = lambda k: np.tile(np.array([0, 0, 1], f32), (k, 1))
        c.add("ndl_ndv_zero", n=zn(keep.sum()), wi=wi[a][keep], wo=wi[b][keep][:, [1, 0, 2]], roughness=rr[keep], metallic=0.5, base=(0.9, 0.6, 0.1), transmission=0.0)
        c.add("ndv_one_ulp", n=zn(one_ulp.sum()), wi=wi[a][one_ulp], wo=wi[b][one_ulp][:, [1, 0, 2]], roughness=rr[one_ulp], metallic=0.5, base=(0.9, 0.6, 0.1), transmission=0.0)
        prod = np.array([0.0009, 0.00099, 0.00101, 0.0011]) / 4
        zl = np.array([0.01, 0.02, 0.05]); a, b = _grid(prod, zl)
        zv = a / b
        c.add("den_001", n=np.tile(np.array([0, 0, 1], f32), (len(a), 1)), wi=np.stack([np.sqrt(1 - b * b), 0 * b, b], 1), wo=np.stack([0 * zv, np.sqrt(1 - zv * zv), zv], 1),
              roughness=0.5, metallic=0.0, base=(1, 1, 1), transmission=0.0)
        t01 = f32(0.01)
        c.add("transmission_001", n=zz, wi=_hemi(g, zz.astype(np.float64), 0.3), wo=_hemi(g, zz.astype(np.float64), 0.3), roughness=0.5, metallic=0.0, base=(1, 1, 1),
              transmission=np.array([t01, np.nextafter(t01, f32(1)), t01, np.nextafter(t01, f32(1))], f32))
        r = np.array(ROUGH[4:], f32); d = np.tile(np.array([0, 0.6, 0.8], f32), (len(r), 1))
        c.add("ndh_at_1", n=d, wi=d, wo=d, roughness=r, metallic=0.0, base=(0.5, 0.5, 0.5), transmission=0.0)
        d = np.tile(np.array([0, 0, 1], f32), (4, 1))
        c.add("ndh_1_rough_0_001", n=d, wi=d, wo=d, roughness=np.array(ROUGH[:4], f32), metallic=0.0, base=(0.5, 0.5, 0.5), transmission=0.0)
    elif op == "unit_vector":
        c.add("bulk", rng=g.integers(0, 2 ** 32, 3001, dtype=np.uint64).astype(np.uint32))
        c.add("draw_edges", rng=np.concatenate([R.pcg_unhash([0, _TOP, 1 << 31]), R.pcg_unhash(R.pcg_unhash([0, _TOP]))]).astype(np.uint32))
    elif op == "sample_bsdf":
        n = 3001
        nr = _unit(g, n); m = _materials(g, n, 0.2)      # (smaller roughness: specular_glossy, specular_rough_005, small_roughness_diffuse, rough0_specular)
        rnd = lambda k: g.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
        c.add("bulk", ffn=nr, wo=_hemi(g, nr.astype(np.float64)), front=1, transmission=0.0, rng=rnd(n), **m)
        n = 600
        nr = _unit(g, n)
        c.add("glass_front", ffn=nr, wo=_hemi(g, nr.astype(np.float64)), front=1, transmission=1.0, ior=g.choice([1.33, 1.5, 2.4], n), base=g.random((n, 3)), rng=rnd(n), roughness=0.0)
        nr = _unit(g, n)
        c.add("glass_back", ffn=nr, wo=_hemi(g, nr.astype(np.float64)), front=0, transmission=1.0, ior=g.choice([1.33, 1.5, 2.4], n), base=g.random((n, 3)), rng=rnd(n), roughness=0.0)
        d = np.array([(0.6, 0, 0.8), (0.36, 0.48, 0.8), (0, 0, 1), (0.6, 0.64, 0.48)], f32)
        c.add("glass_cos_1", ffn=np.tile(d, (2, 1)), wo=np.tile(d, (2, 1)), front=np.repeat([1, 0], len(d)), transmission=1.0, ior=1.5, base=(1, 1, 1), rng=rnd(2 * len(d)), roughness=0.0)
        # back face, ior 1.5: total internal reflection for sin(theta) > 1 / 1.5
        sc = 1 / 1.5
        s = np.array([sc - 1e-2, sc - 1e-3, sc + 1e-3, sc + 1e-2]); s = np.repeat(s, 8)
        c.add("glass_tir_sides", ffn=np.tile(np.array([0, 0, 1], f32), (len(s), 1)), wo=np.stack([s, 0 * s, np.sqrt(1 - s * s)], 1), front=0, transmission=1.0, ior=1.5,
              base=(1, 1, 1), rng=rnd(len(s)), roughness=0.0)
        ks = []
        for ior in (1.5, 1.33, 2.4, 1.1):
            cz = f32(np.sqrt(1 - 1 / float(f32(ior)) ** 2))
            for step in range(-3, 4):
                z = cz
                for _ in range(abs(step)):
                    z = np.nextafter(z, f32(2 if step > 0 else -2))
                ks.append((ior, np.sqrt(max(0.0, 1 - float(z) ** 2)), z))
        ks = np.array(ks)
        c.add("glass_k_negative", ffn=np.tile(np.array([0, 0, 1], f32), (len(ks), 1)), wo=np.stack([ks[:, 1], 0 * ks[:, 1], ks[:, 2]], 1), front=0, transmission=1.0,
              ior=ks[:, 0], base=(1, 1, 1), rng=np.tile(R.pcg_unhash([_TOP]).astype(np.uint32), len(ks)), roughness=0.0)
        # reflectance on both sides of the drawn number: front face, ior 1.5, cos in a grid; the draw crafted around float64's reflectance
        cz = np.repeat(np.array([0.1, 0.3, 0.6, 0.9]), 4)
        refl = R.reflectance(R.E(cz.astype(f32)), R.E(np.full(len(cz), 1 / float(f32(1.5))))).v
        delta = np.tile([-1e-2, -1e-4, 1e-4, 1e-2], 4)
        c.add("glass_reflectance_sides", ffn=np.tile(np.array([0, 0, 1], f32), (len(cz), 1)), wo=np.stack([np.sqrt(1 - cz * cz), 0 * cz, cz], 1), front=1, transmission=1.0,
              ior=1.5, base=(1, 1, 1), rng=_seed_for_draw(refl + delta), roughness=0.0)
        # the first draw on both sides of prob_spec (metallic 0.5, grey: prob_spec well inside its clamps)
        k = 64
        nr = _unit(g, k); wo = _hemi(g, nr.astype(np.float64), 0.2)
        part = np.zeros(k, IN[op]); part["ffn"] = nr; part["wo"] = wo; part["metallic"] = 0.5; part["roughness"] = 0.5; part["base"] = 0.5
        ps = _prob_spec_of(part)
        c.add("prob_spec_sides", ffn=nr, wo=wo, front=1, transmission=0.0, roughness=0.5, metallic=0.5, base=(0.5, 0.5, 0.5),
              rng=_seed_for_draw(ps + np.tile([-1e-2, -1e-4, 1e-4, 1e-2], k // 4)))
        k = 300
        w = _hemi(g, np.repeat(np.array([[0, 0, 1.0]]), k, 0), 0.0).astype(np.float64); w[:, 2] = g.uniform(1e-3, 3e-2, k); w /= np.linalg.norm(w, axis=1, keepdims=True)
        c.add("grazing_below_surface", ffn=np.tile(np.array([0, 0, 1], f32), (k, 1)), wo=w, front=1, transmission=0.0, roughness=g.choice([0.5, 1.0], k), metallic=1.0,
              base=(1, 1, 1), rng=rnd(k))
        k = 40
        nr = _unit(g, k)
        c.add("ndv_negative", ffn=nr, wo=-_hemi(g, nr.astype(np.float64), 0.1), front=1, transmission=0.0, roughness=0.5, metallic=0.0, base=(1, 1, 1), rng=rnd(k))
        r, mt, col = _grid(ROUGH[4:], METAL, np.arange(len(COLOURS)))
        k = len(r); nr = _unit(g, k)
        c.add("materials", ffn=nr, wo=_hemi(g, nr.astype(np.float64), 0.1), front=1, transmission=0.0, roughness=r, metallic=mt, base=np.array(COLOURS, f32)[col], rng=rnd(k))
        # small roughness through the diffuse lobe (first draw 0.9995 > prob_spec <= 0.999): the sampled direction is away from the D peak, where
        # d = n_dot_h^2 (a2 - 1) + 1 is well conditioned; at the peak float64 cannot follow it (ndh_1_rough_0_001 of ndf / eval_*, rough0_specular below)
        r, mt = _grid(ROUGH[:4], METAL)
        k = len(r); nr = _unit(g, k)
        c.add("small_roughness_diffuse", ffn=nr, wo=_hemi(g, nr.astype(np.float64), 0.2), front=1, transmission=0.0, roughness=r, metallic=mt, base=(0.9, 0.6, 0.1),
              rng=_seed_for_draw(np.full(k, 0.9995)))
        # the specular lobe over the glossy range: roughness 0.05, 0.2 and random values in [0.05, 0.5), the first draw below prob_spec. The bound on pdf and
        # weight counts D's error twice (it cancels between bsdf_val and pdf), so float64 leaves about half of such cases undecided; the cap is a condition
        # on the inputs, so candidates are drawn until enough are decided ones, and those are kept.
        k = 12000
        nr = _unit(g, k)
        part = np.zeros(k, IN[op])
        part["ffn"] = nr; part["wo"] = _hemi(g, nr.astype(np.float64), 0.1); part["front"] = 1; part["ior"] = 1.5
        part["roughness"] = np.where(np.arange(k) % 4 == 0, 0.05, np.where(np.arange(k) % 4 == 1, 0.2, g.uniform(0.05, 0.5, k)))
        part["metallic"] = g.choice(METAL, k); part["base"] = g.uniform(0.2, 1.0, (k, 3)); part["rng"] = rnd(k)
        _, first = R.rand_f32(part["rng"].astype(np.uint64))
        _, cand_und = reference(op, part, None)
        ok = np.nonzero((first < _prob_spec_of(part) - 1e-3) & ~cand_und)[0][:1600]
        c.add("specular_glossy", **{name: part[name][ok] for name in part.dtype.names})
        # roughness 0.05 through the specular lobe: d = n_dot_h^2 (a2 - 1) + 1 is then a few a2 = 6e-6 under three roundings of 1, so D is beyond 2^-6 and
        # float64 decides none of these. Kept, all flagged, for the bit equality of the three builds along this chain.
        flagged = np.nonzero((first < _prob_spec_of(part) - 1e-3) & cand_und & (part["roughness"] == f32(0.05)))[0][:400]
        c.add("specular_rough_005", **{name: part[name][flagged] for name in part.dtype.names})
        k = 16                                           # roughness 0 (an out-of-range material id), specular lobe: D = 0 / 0 at the sampled normal
        nr = _unit(g, k)
        c.add("rough0_specular", ffn=nr, wo=_hemi(g, nr.astype(np.float64), 0.2), front=1, transmission=0.0, roughness=0.0, metallic=1.0, base=(1, 1, 1), rng=_seed_for_draw(np.full(k, 0.25)))
    elif op in ("nee0", "nee1"):
        rnd = lambda k: g.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)

        def common(k, **over):
            nr = _unit(g, k); m = _materials(g, k, 0.05)
            f = dict(num_lights=g.choice([1, 3, 100], k), pos=g.uniform(-2, 2, (k, 3)), ffn=nr, wo=_hemi(g, nr.astype(np.float64)), transmission=0.0,
                     visible=g.integers(0, 2, k), rng=rnd(k), **m)
            f.update(over)
            return f
        c.add("bulk", **common(3001))
        # surfaces that face their light: ffn towards the sampled point's side
        f = common(1500)
        idx, lpos, lnrm = _chosen_light(lights, f["num_lights"], f["rng"])
        to = lpos - f["pos"]; to /= np.linalg.norm(to, axis=1, keepdims=True)
        f["ffn"] = (to + 0.5 * _unit(g, 1500)).astype(np.float64); f["ffn"] = (f["ffn"] / np.linalg.norm(f["ffn"], axis=1, keepdims=True)).astype(f32)
        f["wo"] = _hemi(g, f["ffn"].astype(np.float64))
        c.add("facing", **f)
        c.add("draw_is_one", **common(12, rng=np.tile(R.pcg_unhash([_TOP]).astype(np.uint32), 12), num_lights=np.tile([1, 3, 100], 4)))
        c.add("no_lights", **common(12, num_lights=0))
        f = common(200)
        idx, lpos, lnrm = _chosen_light(lights, f["num_lights"], f["rng"])
        to = lpos - f["pos"]; to /= np.linalg.norm(to, axis=1, keepdims=True)
        f["ffn"] = (-to).astype(f32); f["wo"] = _hemi(g, f["ffn"].astype(np.float64))
        c.add("light_behind_surface", **f)
        f = common(200)
        idx, lpos, lnrm = _chosen_light(lights, f["num_lights"], f["rng"])
        ok = np.isfinite(lnrm).all(1)
        f["pos"] = np.where(ok[:, None], lpos - np.where(ok[:, None], lnrm, 0) * g.uniform(0.5, 2.0, (200, 1)), f["pos"]).astype(f32)
        to = lpos - f["pos"]; to /= np.linalg.norm(to, axis=1, keepdims=True)
        f["ffn"] = to.astype(f32); f["wo"] = _hemi(g, f["ffn"].astype(np.float64))
        c.add("surface_behind_light", **f)
        for name, dist in (("tiny_dist_early_out", 9e-5), ("small_dist", 5e-4)):
            f = common(60, visible=np.tile([0, 1], 30), num_lights=1, roughness=g.uniform(0.5, 1.0, 60))      # (L is the normal here: away from small roughness' D peak)
            idx, lpos, lnrm = _chosen_light(lights, f["num_lights"], f["rng"])
            f["ffn"] = (-lnrm).astype(f32); f["pos"] = (lpos + lnrm * (dist + 0.001)).astype(f32); f["wo"] = _hemi(g, f["ffn"].astype(np.float64), 0.2)
            c.add(name, **f)
    elif op == "roulette":
        n = 3001
        rnd = lambda k: g.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
        c.add("bulk", depth=g.integers(1, 8, n), throughput=g.random((n, 3)) * g.choice([0.04, 1.0, 3.0], (n, 1)), ffn=_unit(g, n), next_dir=_unit(g, n),
              pos=g.uniform(-5, 5, (n, 3)), rng=rnd(n))
        d, mx = _grid([2, 3], [0.01, 0.04, 0.5, 0.9, 0.99, 2.0])
        k = len(d)
        thr = np.stack([mx, mx * 0.5, mx * 0.25], 1)[:, [1, 0, 2]]
        c.add("depth_and_maxima", depth=d, throughput=thr, ffn=_unit(g, k), next_dir=_unit(g, k), pos=g.uniform(-5, 5, (k, 3)), rng=rnd(k))
        mx = np.repeat([0.01, 0.3, 0.6, 0.99], 4); surv = np.clip(mx.astype(f32).astype(np.float64), float(f32(0.05)), float(f32(0.95)))
        k = len(mx)
        c.add("draw_sides", depth=3, throughput=np.stack([mx, mx, mx], 1), ffn=_unit(g, k), next_dir=_unit(g, k), pos=g.uniform(-5, 5, (k, 3)),
              rng=_seed_for_draw(surv + np.tile([-1e-2, -1e-4, 1e-4, 1e-2], 4)))
        c.add("draw_equals_survival", depth=np.array([3, 5], np.uint32), throughput=np.full((2, 3), 0.5, f32), ffn=_unit(g, 2), next_dir=_unit(g, 2), pos=g.uniform(-5, 5, (2, 3)),
              rng=np.tile(R.pcg_unhash([1 << 31]).astype(np.uint32), 2))
        z = np.tile(np.array([0, 0, 1], f32), (6, 1))
        nd = np.array([(1, 0, 0), (0, -1, 0), (0.6, 0.8, 0), (0, 0.6, 0.8), (0, 0.6, -0.8), (0.6, 0.8, -0.0)], f32)
        c.add("offset_sign", depth=np.array([1, 2, 3, 1, 2, 1], np.uint32), throughput=np.full((6, 3), 0.97, f32), ffn=z, next_dir=nd, pos=g.uniform(-5, 5, (6, 3)), rng=rnd(6))
    else:
        raise KeyError(op)
    return c.done()


def _prob_spec_of(part):
    """float64's prob_spec of sample_bsdf records (for crafting the first draw around it)."""
    n = len(part)
    ffn, wo, base = R.vec(part["ffn"]), R.vec(part["wo"]), R.vec(part["base"])
    metal = R.E(part["metallic"])
    F0 = R.mix3(tuple(R.E(np.full(n, R.L(0.04))) for _ in range(3)), base, metal)
    return R._prob_spec(R.fresnel_schlick(F0, R.maxE(R.dot(ffn, wo), 0.0)), base, metal, ()).v


def _chosen_light(lights, num_lights, rng):
    """Which light a nee record samples, and float64's sampled point and normal on it (for crafting the geometry around it)."""
    n = len(rng)
    rng1, r0 = R.rand_f32(np.asarray(rng, np.uint64))
    nl = np.asarray(num_lights, np.int64)
    idx = np.minimum((r0 * nl.astype(f32)).astype(f32).astype(np.int64), np.maximum(nl - 1, 0))
    _, pos, nrm, _, _ = R.sample_light(lights[idx], rng1, R.Und(n))
    return idx, np.stack([p.v for p in pos], 1), np.stack([p.v for p in nrm], 1)


_CACHE = {}


def prepared(op):
    """(inp, groups, lights, float64 outputs, undecided), computed once per process and not modified by the tests."""
    if op not in _CACHE:
        lights = light_table()
        inp, groups = cases(op, lights)
        ref, und = reference(op, inp, lights)
        _CACHE[op] = (inp, groups, lights, ref, und)
    return _CACHE[op]
