"""Float64 restatement of the shading arithmetic of trace_path, written from restir.wgsl alone (and restir_spatial.wgsl:380-400 for the one place the
spatial variant differs: trace_shadow_ray's t_min and its early-out). Line numbers are restir.wgsl's. Nothing here is shared with the product (csrc/)
or the oracle (oracle/).

  pcg_hash / rand :132-141          random_unit_vector :143-150      make_orthonormal_basis :161-168     fresnel_schlick :170
  reflectance :175                  ndf_ggx :182                     geometry_schlick_ggx / geometry_smith :189-200
  sample_ggx_vndf :202-216          sample_light :219-245            eval_pdf :249-276                   eval_bsdf :278-305
  sample_bsdf :307-371              eval_direct_lighting :443-459 (its ray's answer an input)            the NEE block :558-571
  roulette and ray offset :593-603

Conventions (those of _wgsl_f64_restir.py). Integer work is exact u32 arithmetic. rand() returns the f32 value the shader forms: the literal
4294967295.0 is 2^32 as an f32, so rand() = f32(rng_seed) * 2^-32, exactly 1.0 for the top 128 seeds. Shader literals enter with their f32 values
(L(x)). Values that only choose a branch or an index are formed in f32 as the shader forms them (u32(rand() * f32(num_lights))). Everything that
flows into an output is float64, with the true sin, cos and sqrt. WGSL builtins follow DESIGN.md §3: min, max and clamp with a NaN operand return the
other operand (clamp(NaN, lo, hi) = lo); reflect(I, N) = I - 2 dot(N, I) N; refract(I, N, eta) = 0 if k = 1 - eta^2 (1 - dot(N, I)^2) < 0, else
eta I - (eta dot(N, I) + sqrt(k)) N; sign(0) = 0; pow(x, 5) is the fifth power.

Bounds are derived, not measured: every value is carried as E(v, e, r) — the float64 value, a bound e on |f32 result - v| and r, the largest
single rounding's contribution to e (carried through the same conditioning): e / r says how many roundings of comparable weight the bound is made of. Each operation propagates the bounds of its operands through its own conditioning (a product |a| e_b + |b| e_a + e_a e_b; a
quotient (e_a + |a / b| e_b) / (|b| - e_b); a square root sqrt(x) - sqrt(x - e_x); so a cosine's absolute error is divided by what it is divided by,
ndf_ggx's d = n_dot_h^2 (a2 - 1) + 1 carries 1 / d twice into D, and 1 - cos^2 under a root carries its cancellation) and adds its own rounding:
2^-24 of the magnitude of its result (a division counts twice: an implementation may evaluate a / b as a * (1 / b)). The polynomial sin / cos enter
with the 2e-7 absolute error tests/test_oracle_kat.py holds them to, on top of the propagated error of their argument. A comparison is undecided when
its two sides are closer than their bounds plus BAND (relative); a case is undecided when a comparison it reaches is, when a value is not finite in
float64 or its bound is not, or when an output's bound exceeds 2^-6 of its magnitude (of its vector's largest component).

`mis` (a set of names) applies one deliberate misreading to this side only (tests/test_wgsl_f64_sensitivity.py):
  "g1_alpha2"             a2 = roughness^4 in geometry_schlick_ggx (:194)      "prob_spec_swapped"     lum_diff in the numerator (:263, :334)
  "fresnel_n_dot_v"       F of eval_bsdf from n_dot_v (:296)                   "pdf_g_smith"           geometry_smith in pdf_spec (:269-270)
  "kd_no_metallic"        (1 - metallic) dropped from kD (:301)                "glass_ratio_swapped"   select arguments exchanged (:315)
  "glass_no_short_circuit" the draw of :318 always taken                       "vndf_no_stretch_back"  alpha dropped in the final normalize (:215)
  "sphere_radius_u"       light.u.x for the radius (:240)                      "mis_power"             power heuristic (:565)
  "nee_tmax_dist"         t_max = dist (:377)                                  "nee_pdf_from_offset"   p_bsdf from offset_pos (:564)
  "roulette_ge"           rand() >= survival_prob (:596)                       "offset_no_sign"        offset always along +ffnormal (:602)
"""
import numpy as np

f32 = np.float32
EPS = 2.0 ** -24
BAND = 16 * EPS                      # as _wgsl_f64_restir.py
REL_LIMIT = 2.0 ** -6
TRIG_ABS = 2e-7                      # tests/test_oracle_kat.py: the polynomial sin / cos on [0, 2 pi]
_MASK = np.uint64(0xFFFFFFFF)
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def L(x):
    """A shader literal: its f32 value, as float64."""
    return float(f32(x))


PI = L(3.14159265359)                # :4
LUM = (L(0.2126), L(0.7152), L(0.0722))


def pcg_hash(x):                     # :132-136
    x = np.asarray(x, np.uint64) & _MASK
    state = (x * np.uint64(747796405) + np.uint64(2891336453)) & _MASK
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & _MASK
    return ((word >> np.uint64(22)) ^ word) & _MASK


def pcg_unhash(y):
    """The inverse of pcg_hash (a bijection of u32: an affine step, then the RXS-M-XS output permutation). For crafting a case's first draw."""
    y = np.asarray(y, np.uint64) & _MASK
    word = y ^ (y >> np.uint64(22))                                       # undo the xorshift by 22 (one round suffices: 2 * 22 >= 32)
    word = (word * np.uint64(pow(277803737, -1, 1 << 32))) & _MASK
    shift = (word >> np.uint64(28)) + np.uint64(4)                        # the top four bits survive state ^ (state >> shift), shift >= 4
    state = word.copy()
    for _ in range(8):
        state = word ^ (state >> shift)
    return ((state - np.uint64(2891336453)) * np.uint64(pow(747796405, -1, 1 << 32))) & _MASK


def rand_f32(rng):
    """rand() :138-141 -> (new state, the f32 value). f32(u32) rounds to nearest; dividing by 2^32 is exact."""
    rng = pcg_hash(rng)
    return rng, (rng.astype(np.uint32).astype(f32) / f32(4294967295.0)).astype(f32)


# ------------------------------------------------------------------------------------------------ values with bounds
class E:
    __slots__ = ("v", "e", "n")

    def __init__(self, v, e=0.0, n=0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)
        self.n = np.broadcast_to(np.asarray(n, np.float64), self.v.shape)      # (r of the docstring)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def _round(self, v, e, n, k=1):
        with np.errstate(**_ERR):
            mag = np.abs(v) + e
            tiny = np.where((mag < 2.0 ** -125) & (mag > 0), 2.0 ** -149, 0.0)      # a denormal result rounds absolutely
            # exact operands and a result that is an f32: a correctly rounded operation returns it, no rounding (not for a / b taken as a * (1 / b))
            exact = (e == 0) & (v.astype(f32).astype(np.float64) == v) if k == 1 else False
            return E(v, np.where(exact, 0.0, e + k * EPS * mag + tiny), np.where(exact, 0.0, np.maximum(n, EPS * mag + tiny)))

    def __add__(self, o):
        o = E.of(o)
        with np.errstate(**_ERR):
            return self._round(self.v + o.v, self.e + o.e, np.maximum(self.n, o.n))
    __radd__ = __add__

    def __neg__(self):
        return E(-self.v, self.e, self.n)

    def __sub__(self, o):
        return self + (-E.of(o))

    def __rsub__(self, o):
        return E.of(o) + (-self)

    def __mul__(self, o):
        o = E.of(o)
        with np.errstate(**_ERR):
            return self._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e,
                               (np.abs(self.v) + self.e) * o.n + (np.abs(o.v) + o.e) * self.n)      # (a sum: x * x carries x's rounding twice)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.of(o)
        with np.errstate(**_ERR):
            v = self.v / o.v
            den = np.abs(o.v) - o.e
            e = np.where(den > 0, (self.e + np.abs(v) * o.e) / den, np.inf)
            e = np.where((self.e == 0) & (o.e == 0), 0.0, e)
            r = np.where(den > 0, np.maximum(self.n, np.abs(v) * o.n) / den, np.inf)
            return self._round(v, e, r, 2)

    def __rtruediv__(self, o):
        return E.of(o) / self


def sqrt(x, floor0=False):
    """floor0: the argument went through max(0, .), so its true value is not below 0 whatever its bound says."""
    with np.errstate(**_ERR):
        v = np.sqrt(x.v)
        lo = x.v - x.e
        e = np.maximum(v - np.sqrt(np.maximum(lo, 0.0)), np.sqrt(x.v + x.e) - v)
        if not floor0:
            e = np.where((lo < 0) & (x.e > 0), np.inf, e)                 # the f32 argument may be negative: NaN
        return x._round(v, e, np.where(x.e > 0, x.n * (e / x.e), 0.0))


def _pick(take_b, a, b):
    return np.where(take_b, b, a)


def maxE(a, b):
    """WGSL max: a NaN operand is dropped."""
    a, b = E.of(a), E.of(b)
    with np.errstate(**_ERR):
        tb = np.isnan(a.v) | (b.v > a.v)
        tb &= ~np.isnan(b.v)
        both = ~np.isnan(a.v) & ~np.isnan(b.v) & (np.abs(a.v - b.v) <= a.e + b.e)
        return E(_pick(tb, a.v, b.v), np.where(both, np.maximum(a.e, b.e), _pick(tb, a.e, b.e)), _pick(tb, a.n, b.n))


def minE(a, b):
    return -maxE(-E.of(a), -E.of(b))


def clampE(x, lo, hi):
    return minE(maxE(x, lo), hi)


def sel(c, a, b):
    """select(b, a, c) on values with bounds: a where c."""
    a, b = E.of(a), E.of(b)
    return E(np.where(c, a.v, b.v), np.where(c, a.e, b.e), np.where(c, a.n, b.n))


def sincos(x):
    with np.errstate(**_ERR):
        r = np.maximum(x.n, TRIG_ABS)
        return (E(np.sin(x.v), x.e + TRIG_ABS, r), E(np.cos(x.v), x.e + TRIG_ABS, r))


class Und:
    """The undecided flag of a batch of cases."""

    def __init__(self, n):
        self.f = np.zeros(n, bool)

    def gt(self, a, b, live=True):
        """a > b; flags the live cases whose comparison float64 cannot settle."""
        a, b = E.of(a), E.of(b)
        with np.errstate(**_ERR):
            d = a.v - b.v
            band = a.e + b.e + BAND * np.maximum(np.abs(a.v), np.abs(b.v))
            band = np.where((a.e == 0) & (b.e == 0), 0.0, band)           # both sides exact: the comparison is
            und = ~np.isfinite(d) | ~np.isfinite(band) | ((np.abs(d) <= band) & (band > 0))
            self.f |= und & live
            return d > 0

    def mark(self, cond, live=True):
        self.f |= cond & live


# vectors: tuples of three E
def vec(a):
    a = np.asarray(a)
    return tuple(E(a[..., k]) for k in range(3))


def vadd(a, b): return tuple(x + y for x, y in zip(a, b))
def vsub(a, b): return tuple(x - y for x, y in zip(a, b))
def vneg(a): return tuple(-x for x in a)
def vscale(a, s): return tuple(x * s for x in a)
def vmul(a, b): return tuple(x * y for x, y in zip(a, b))
def vsel(c, a, b): return tuple(sel(c, x, y) for x, y in zip(a, b))
def dot(a, b): return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
def cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
def length(a): return sqrt(dot(a, a), floor0=True)
def normalize(a): return vscale(a, 1.0 / length(a))
def vdiv(a, s): r = 1.0 / E.of(s); return vscale(a, r)
def reflect(i, n): return vsub(i, vscale(n, 2.0 * dot(n, i)))
def luminance(c): return (c[0] * LUM[0] + c[1] * LUM[1]) + c[2] * LUM[2]      # :742
def mix3(a, b, t): return vadd(vscale(a, 1.0 - t), vscale(b, t))
def zero3(n): return tuple(E(np.zeros(n)) for _ in range(3))


def dot_normalized(nrm, v):
    """dot(nrm, normalize(v)) with the bound a cosine deserves. Component-wise propagation treats an error of v as if it could point anywhere, so at
    n_dot_h near 1 it charges the cosine with the whole direction error of h. Geometrically an error dv of v turns h by at most |dv| / |v| and moves
    dot(nrm, h) by that angle times the part of nrm ACROSS h, sqrt(|nrm|^2 - c^2), plus half its square; along h only normalize's own roundings act
    (dot 3, sqrt 1, reciprocal 1, product 1: 6), scaled by c. Added: nrm's own error and the 3 roundings of the final dot. Both bounds hold; the
    smaller is kept."""
    generic = dot(nrm, normalize(v))
    with np.errstate(**_ERR):
        dv = np.sqrt(sum(c.e ** 2 for c in v))
        lv = np.sqrt(sum(c.v ** 2 for c in v))
        dn = np.sqrt(sum(c.e ** 2 for c in nrm))
        n2 = sum(c.v ** 2 for c in nrm)
        turn = np.where(lv > dv, dv / (lv - dv), np.inf) + 6 * EPS
        h = [c.v / lv for c in v]
        cval = sum(a.v * b for a, b in zip(nrm, h))
        across = np.sqrt(np.maximum(n2 - cval ** 2, 0.0))
        e = across * turn + np.sqrt(n2) * turn ** 2 + np.abs(cval) * 6 * EPS + dn * (1 + turn) + 3 * EPS * sum(np.abs(a.v * b) for a, b in zip(nrm, h))
        e = np.where(np.isfinite(e), np.minimum(e, generic.e), generic.e)
    return E(generic.v, e, np.minimum(generic.n, e))


def pow5(x):
    x2 = x * x
    return (x2 * x2) * x


# ------------------------------------------------------------------------------------------------ the functions
def make_orthonormal_basis(n, U, live=True):                              # :161-168
    pos = ~U.gt(0.0, n[2], live)                                          # n.z >= 0
    sign = E(np.where(pos, 1.0, -1.0))
    a = -1.0 / (sign + n[2])
    b = n[0] * n[1] * a
    t = (1.0 + sign * n[0] * n[0] * a, sign * b, -sign * n[0])
    bt = (b, sign + n[1] * n[1] * a, -n[1])
    return t, bt


def fresnel_schlick(f0, v_dot_h):                                         # :170
    p = pow5(clampE(1.0 - v_dot_h, 0.0, 1.0))
    return tuple(f + (1.0 - f) * p for f in f0)


def reflectance(cosine, ref_idx):                                         # :175
    r0 = (1.0 - ref_idx) / (1.0 + ref_idx)
    r0 = r0 * r0
    return r0 + (1.0 - r0) * pow5(1.0 - cosine)


def ndf_ggx(n_dot_h, roughness):                                          # :182
    a = roughness * roughness
    a2 = a * a
    d = n_dot_h * n_dot_h * (a2 - 1.0) + 1.0
    return a2 / (PI * d * d)


def geometry_schlick_ggx(n_dot_v, roughness, mis=()):                     # :189
    a2 = roughness * roughness
    if "g1_alpha2" in mis:
        a2 = a2 * a2
    return 2.0 * n_dot_v / (n_dot_v + sqrt(a2 + (1.0 - a2) * n_dot_v * n_dot_v))


def geometry_smith(n_dot_l, n_dot_v, roughness, mis=()):                  # :198
    return geometry_schlick_ggx(n_dot_l, roughness, mis) * geometry_schlick_ggx(n_dot_v, roughness, mis)


def sample_ggx_vndf(wo, roughness, ux, uy, U, live=True, mis=()):         # :202-216
    alpha = roughness * roughness
    Vh = normalize((alpha * wo[0], alpha * wo[1], wo[2]))
    lensq = Vh[0] * Vh[0] + Vh[1] * Vh[1]
    has = U.gt(lensq, 0.0, live)
    inv = 1.0 / sqrt(lensq, floor0=True)
    T1 = vsel(has, (-Vh[1] * inv, Vh[0] * inv, E(np.zeros_like(lensq.v)) * inv), (E(np.ones_like(lensq.v)), E(np.zeros_like(lensq.v)), E(np.zeros_like(lensq.v))))
    T2 = cross(Vh, T1)
    r = sqrt(E.of(ux))
    phi = 2.0 * PI * E.of(uy)
    sphi, cphi = sincos(phi)
    t1 = r * cphi
    t2 = r * sphi
    s = 0.5 * (1.0 + Vh[2])
    t2l = (1.0 - s) * sqrt(1.0 - t1 * t1) + s * t2
    w = sqrt(maxE(0.0, 1.0 - t1 * t1 - t2l * t2l), floor0=True)
    Nh = vadd(vadd(vscale(T1, t1), vscale(T2, t2l)), vscale(Vh, w))
    if "vndf_no_stretch_back" in mis:
        return normalize((Nh[0], Nh[1], maxE(0.0, Nh[2])))
    return normalize((alpha * Nh[0], alpha * Nh[1], maxE(0.0, Nh[2])))


def random_unit_vector(rng):                                              # :143-150 -> (rng, vector)
    rng, r1 = rand_f32(rng)
    rng, r2 = rand_f32(rng)
    z = E(r1) * 2.0 - 1.0
    a = E(r2) * 2.0 * PI
    r = sqrt(1.0 - z * z, floor0=True)                                    # |z| <= 1 in f32 as well (rand() is in [0, 1]): the argument is never negative
    sa, ca = sincos(a)
    return rng, (r * ca, r * sa, z)


def sample_light(light, rng, U, live=True, mis=()):                       # :219-245 -> (rng, pos, normal, pdf, emission)
    """light: structured array of the 64-byte light records (position, type, u, area, v, pad, emission)."""
    rng, r1 = rand_f32(rng)
    rng, r2 = rand_f32(rng)
    r1, r2 = E(r1), E(r2)
    lp, lu, lv = vec(light["position"]), vec(light["u"]), vec(light["v"])
    quad = light["type"] == 0
    su = r1 * 2.0 - 1.0
    sv = r2 * 2.0 - 1.0
    q_pos = vadd(vadd(lp, vscale(lu, su)), vscale(lv, sv))
    q_n = normalize(cross(lu, lv))
    z = 1.0 - 2.0 * r1
    r_xy = sqrt(maxE(0.0, 1.0 - z * z), floor0=True)
    phi = 2.0 * PI * r2
    sp, cp = sincos(phi)
    ld = (r_xy * cp, r_xy * sp, z)
    radius = lu[0] if "sphere_radius_u" in mis else lv[0]
    s_pos = vadd(lp, vscale(ld, radius))
    pdf = 1.0 / E(light["area"])
    return rng, vsel(quad, q_pos, s_pos), vsel(quad, q_n, ld), pdf, light["emission"]


def _prob_spec(F, base, metallic, mis):
    lum_spec = luminance(F)
    lum_diff = luminance(vscale(base, 1.0 - metallic))
    num = lum_diff if "prob_spec_swapped" in mis else lum_spec
    return clampE(num / (lum_spec + lum_diff + L(0.0001)), L(0.001), L(0.999))


def eval_pdf(normal, wi, wo, m, base, U, live=True, mis=()):             # :249-276
    n_dot_l = dot(normal, wi)
    n_dot_v = dot(normal, wo)
    glass = np.asarray(m["transmission"], f32) > f32(0.01)
    live = live & ~glass
    below = ~U.gt(n_dot_l, 0.0, live)
    below |= ~U.gt(n_dot_v, 0.0, live & ~below)
    live = live & ~below
    rough, metal = E(m["roughness"]), E(m["metallic"])
    F0 = mix3(tuple(E(np.full_like(rough.v, L(0.04))) for _ in range(3)), base, metal)
    F = fresnel_schlick(F0, maxE(dot(normal, wo), 0.0))
    prob_spec = _prob_spec(F, base, metal, mis)
    n_dot_h = maxE(dot_normalized(normal, vadd(wi, wo)), 0.0)            # h = normalize(wi + wo), :266-267
    d = ndf_ggx(n_dot_h, rough)
    g1 = geometry_smith(n_dot_l, n_dot_v, rough, mis) if "pdf_g_smith" in mis else geometry_schlick_ggx(n_dot_v, rough, mis)
    pdf_spec = (d * g1) / (4.0 * n_dot_v)
    pdf_diff = maxE(n_dot_l, 0.0) / PI
    pdf = prob_spec * pdf_spec + (1.0 - prob_spec) * pdf_diff
    return sel(glass | below, 0.0, pdf)


def eval_bsdf(normal, wi, wo, m, base, U, live=True, mis=()):            # :278-305
    n_dot_l = dot(normal, wi)
    n_dot_v = dot(normal, wo)
    glass = np.asarray(m["transmission"], f32) > f32(0.01)
    live = live & ~glass
    below = ~U.gt(n_dot_l, 0.0, live)
    below |= ~U.gt(n_dot_v, 0.0, live & ~below)
    rough, metal = E(m["roughness"]), E(m["metallic"])
    h = normalize(vadd(wi, wo))
    n_dot_h = maxE(dot_normalized(normal, vadd(wi, wo)), 0.0)
    h_dot_v = maxE(dot(h, wo), 0.0)
    F0 = mix3(tuple(E(np.full_like(rough.v, L(0.04))) for _ in range(3)), base, metal)
    D = ndf_ggx(n_dot_h, rough)
    G = geometry_smith(n_dot_l, n_dot_v, rough, mis)
    F = fresnel_schlick(F0, maxE(n_dot_v, 0.0) if "fresnel_n_dot_v" in mis else h_dot_v)
    den = maxE(4.0 * n_dot_l * n_dot_v, L(0.001))
    specular = vdiv(vscale(F, D * G), den)                                # (D * G * F) / max(...)
    kD = tuple(1.0 - f for f in F) if "kd_no_metallic" in mis else vscale(tuple(1.0 - f for f in F), 1.0 - metal)
    diffuse = vdiv(vmul(kD, base), PI)
    out = vadd(diffuse, specular)
    return vsel(glass | below, zero3(len(glass)), out)


def sample_bsdf(wo, ffn, front, m, base, rng, U, mis=()):                 # :307-371 -> (rng, wi, pdf, weight)
    n = len(rng)
    rng0 = np.asarray(rng, np.uint64)
    glass = np.asarray(m["transmission"], f32) > f32(0.01)
    # glass :312-325
    ior = E(m["ior"])
    front = np.asarray(front, bool)
    ratio = sel(~front if "glass_ratio_swapped" in mis else front, 1.0 / ior, ior)      # :315
    cos_theta = minE(dot(wo, ffn), 1.0)
    sin_theta = sqrt(1.0 - cos_theta * cos_theta, floor0=True)            # cos_theta <= 1 by the min (and > -1 for wo on the ffnormal's side): never negative
    total = U.gt(ratio * sin_theta, 1.0, glass)
    rng_g, rg = rand_f32(rng0)
    drew = glass & (np.ones(n, bool) if "glass_no_short_circuit" in mis else ~total)    # :318: || short-circuits
    refl = total | U.gt(reflectance(cos_theta, ratio), E(rg), drew & ~total)
    i = vneg(wo)
    ndi = dot(ffn, i)
    k = 1.0 - ratio * ratio * (1.0 - ndi * ndi)
    kneg = U.gt(0.0, k, glass & ~refl)
    refr = vsub(vscale(i, ratio), vscale(ffn, ratio * ndi + sqrt(maxE(k, 0.0), floor0=True)))
    g_wi = vsel(refl, reflect(i, ffn), vsel(kneg, zero3(n), refr))
    # opaque :328-368
    live = ~glass
    rough, metal = E(m["roughness"]), E(m["metallic"])
    F0 = mix3(tuple(E(np.full(n, L(0.04))) for _ in range(3)), base, metal)
    F_view = fresnel_schlick(F0, maxE(dot(ffn, wo), 0.0))
    prob_spec = _prob_spec(F_view, base, metal, mis)
    rng1, rnd = rand_f32(rng0)
    spec = U.gt(prob_spec, E(rnd), live)                                  # rnd < prob_spec
    t, bt = make_orthonormal_basis(ffn, U, live & spec)
    wo_local = (dot(t, wo), dot(bt, wo), dot(ffn, wo))                    # transpose(tbn) * wo
    rng2, ru = rand_f32(rng1)
    rng3, rv = rand_f32(rng2)
    wm_l = sample_ggx_vndf(wo_local, rough, ru, rv, U, live & spec, mis)
    wm = vadd(vadd(vscale(t, wm_l[0]), vscale(bt, wm_l[1])), vscale(ffn, wm_l[2]))      # tbn * wm_local
    s_wi = reflect(i, wm)
    rng3d, ruv = random_unit_vector(rng1)
    d_wi = normalize(vadd(ffn, ruv))
    wi = vsel(spec, s_wi, d_wi)
    n_dot_l = dot(ffn, wi)
    n_dot_v = dot(ffn, wo)
    below = ~U.gt(n_dot_l, 0.0, live)
    below |= ~U.gt(n_dot_v, 0.0, live & ~below)
    live2 = live & ~below
    bsdf_val = eval_bsdf(ffn, wi, wo, m, base, U, live2, mis)
    pdf = eval_pdf(ffn, wi, wo, m, base, U, live2, mis)
    has = U.gt(pdf, 0.0, live2)
    weight = vdiv(vscale(bsdf_val, n_dot_l), pdf)
    zero = below | ~has
    o_wi = vsel(glass, g_wi, wi)
    o_pdf = sel(glass | zero, 0.0, pdf)
    o_w = vsel(glass, base, vsel(zero, zero3(n), weight))
    o_rng = np.where(glass, np.where(drew, rng_g, rng0), rng3)
    return o_rng, o_wi, o_pdf, o_w


def nee(variant, lights, num_lights, pos, ffn, wo, m, base, visible, rng, U, mis=()):
    """The NEE block :558-571 with eval_direct_lighting :443-459 and trace_shadow_ray (:375-381; variant 1: restir_spatial.wgsl:380-400), the ray's
    answer given. -> dict: nee (0 skipped, 1 no ray and no light, 2 a ray, 3 lit without a ray), want, o, d, tmin, tmax, direct, rng."""
    n = len(rng)
    rng0 = np.asarray(rng, np.uint64)
    nl = np.asarray(num_lights, np.int64)
    some = nl > 0                                                         # :558
    rng1, r0 = rand_f32(rng0)
    idx = (r0 * nl.astype(f32)).astype(f32).astype(np.int64)              # :559, formed in f32
    inside = some & (idx < nl)                                            # :560
    light = lights[np.where(inside, idx, 0)]
    rng3, l_pos, l_n, l_pdf, emission = sample_light(light, rng1, U, inside, mis)
    pdf_nee = l_pdf * (1.0 / E(np.maximum(nl, 1).astype(np.float64)))     # :563 (f32(num_lights) is exact)
    offset_pos = vadd(pos, vscale(ffn, L(0.001)))                         # :444
    from_ = offset_pos if "nee_pdf_from_offset" in mis else pos
    p_bsdf = eval_pdf(ffn, normalize(vsub(l_pos, from_)), wo, m, base, U, inside, mis)   # :564
    if "mis_power" in mis:
        mis_w = (pdf_nee * pdf_nee) / (pdf_nee * pdf_nee + p_bsdf * p_bsdf)
    else:
        mis_w = pdf_nee / (pdf_nee + p_bsdf)                              # :565
    weight = mis_w / pdf_nee                                              # :567
    to = vsub(l_pos, offset_pos)
    Ld = normalize(to)                                                    # :445
    dist = length(to)                                                     # :446
    n_dot_l = maxE(dot(ffn, Ld), 0.0)
    l_dot_n = maxE(dot(vneg(Ld), l_n), 0.0)
    facing = U.gt(n_dot_l, 0.0, inside)
    facing &= U.gt(l_dot_n, 0.0, inside & facing)                         # :451
    reach = inside & facing
    t_max = maxE(dist * (1.0 if "nee_tmax_dist" in mis else L(0.999)), 0.0)   # :377
    t_min = L(0.001) if variant == 0 else L(0.0001)
    early = np.zeros(n, bool)
    if variant == 1:
        early = reach & ~U.gt(t_max, t_min, reach)                        # t_min >= t_max: lit without a ray
    ray = reach & ~early
    lit = early | (ray & np.asarray(visible, bool))
    f = eval_bsdf(ffn, Ld, wo, m, base, U, lit, mis)                      # :453
    G = (n_dot_l * l_dot_n) / (dist * dist)                               # :454
    Le = vscale(vec(emission[..., :3]), E(emission[..., 3]))
    direct = vscale(vscale(vmul(Le, f), G), weight)                       # :455
    z3 = zero3(n)
    return {"nee": np.where(~inside, 0, np.where(~facing, 1, np.where(early, 3, 2))), "want": ray.astype(np.int64),
            "o": vsel(ray, offset_pos, z3), "d": vsel(ray, Ld, z3), "tmin": sel(ray, t_min, 0.0), "tmax": sel(ray, t_max, 0.0),
            "direct": vsel(lit, direct, z3), "rng": np.where(inside, rng3, np.where(some, rng1, rng0))}


def roulette(depth, throughput, ffn, next_dir, pos, rng, U, mis=()):      # :593-603 -> dict: survived, throughput, origin, rng
    n = len(rng)
    rng0 = np.asarray(rng, np.uint64)
    deep = np.asarray(depth, np.int64) >= 3
    p = maxE(throughput[0], maxE(throughput[1], throughput[2]))
    surv = clampE(p, L(0.05), L(0.95))
    rng1, r = rand_f32(rng0)
    if "roulette_ge" in mis:
        dead = deep & ~U.gt(surv, E(r), deep)
    else:
        dead = deep & U.gt(E(r), surv, deep)                              # :596
    thr = vsel(deep, vdiv(throughput, surv), throughput)                  # :597
    sd = dot(ffn, next_dir)
    sgn = np.where(U.gt(sd, 0.0, ~dead), 1.0, np.where(U.gt(0.0, sd, ~dead), -1.0, 0.0))   # sign(), :602
    if "offset_no_sign" in mis:
        sgn = np.ones(n)
    origin = vadd(pos, vscale(vscale(ffn, E(sgn)), L(0.001)))             # :603
    z3 = zero3(n)
    return {"survived": (~dead).astype(np.int64), "throughput": vsel(dead, throughput, thr), "origin": vsel(dead, z3, origin),
            "rng": np.where(deep, rng1, rng0)}
