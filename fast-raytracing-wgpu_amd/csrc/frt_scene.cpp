// frt_scene.cpp — host scene model, geometry generators, scene factories, camera.
// Mirrors src/geometry.rs, src/scene/{builder,material,scenes}.rs, src/camera.rs; matrix helpers follow glam 0.30.9
// (Cargo.lock:876), f32 throughout.
#include "frt_scene.hpp"
#include "frt_vertex_normal.hpp"      // encode_vertex_normal, recomputed_vertex_normal: shared with the device
#include "frt_skin.hpp"               // skinned_position: shared with the device
#include "frt_morph.hpp"              // morphed_position: shared with the device
#include <cmath>
#include <cstring>
#include <map>
#include <algorithm>

namespace frt {

// ---------------------------------------------------------------------------------------------- Mat4 (glam)
Mat4 mat4_identity() { Mat4 r{}; r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.0f; return r; }
Mat4 mat4_mul(const Mat4& a, const Mat4& b) {
    // glam Mat4 * Mat4: column j = ((a.x*b.x + a.y*b.y) + a.z*b.z) + a.w*b.w
    Mat4 r;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i)
            r.m[4 * j + i] = ((a.m[i] * b.m[4 * j] + a.m[4 + i] * b.m[4 * j + 1]) + a.m[8 + i] * b.m[4 * j + 2]) + a.m[12 + i] * b.m[4 * j + 3];
    return r;
}
Mat4 mat4_translation(float x, float y, float z) { Mat4 r = mat4_identity(); r.m[12] = x; r.m[13] = y; r.m[14] = z; return r; }
Mat4 mat4_scale(float x, float y, float z) { Mat4 r = mat4_identity(); r.m[0] = x; r.m[5] = y; r.m[10] = z; return r; }
Mat4 mat4_rotation_x(float a) { float s = sinf(a), c = cosf(a); Mat4 r = mat4_identity(); r.m[5] = c; r.m[6] = s; r.m[9] = -s; r.m[10] = c; return r; }
Mat4 mat4_rotation_y(float a) { float s = sinf(a), c = cosf(a); Mat4 r = mat4_identity(); r.m[0] = c; r.m[2] = -s; r.m[8] = s; r.m[10] = c; return r; }
Mat4 mat4_rotation_z(float a) { float s = sinf(a), c = cosf(a); Mat4 r = mat4_identity(); r.m[0] = c; r.m[1] = s; r.m[4] = -s; r.m[5] = c; return r; }
Mat4 mat4_inverse(const Mat4& a) {
    // glam scalar Mat4::inverse: 2x2 sub-determinants ("coef"), four cofactor rows, sign masks, 1/det
    const float* m = a.m;
    auto M = [&](int c, int r) { return m[4 * c + r]; };
    float c00 = M(2, 2) * M(3, 3) - M(3, 2) * M(2, 3), c02 = M(1, 2) * M(3, 3) - M(3, 2) * M(1, 3), c03 = M(1, 2) * M(2, 3) - M(2, 2) * M(1, 3);
    float c04 = M(2, 1) * M(3, 3) - M(3, 1) * M(2, 3), c06 = M(1, 1) * M(3, 3) - M(3, 1) * M(1, 3), c07 = M(1, 1) * M(2, 3) - M(2, 1) * M(1, 3);
    float c08 = M(2, 1) * M(3, 2) - M(3, 1) * M(2, 2), c10 = M(1, 1) * M(3, 2) - M(3, 1) * M(1, 2), c11 = M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2);
    float c12 = M(2, 0) * M(3, 3) - M(3, 0) * M(2, 3), c14 = M(1, 0) * M(3, 3) - M(3, 0) * M(1, 3), c15 = M(1, 0) * M(2, 3) - M(2, 0) * M(1, 3);
    float c16 = M(2, 0) * M(3, 2) - M(3, 0) * M(2, 2), c18 = M(1, 0) * M(3, 2) - M(3, 0) * M(1, 2), c19 = M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2);
    float c20 = M(2, 0) * M(3, 1) - M(3, 0) * M(2, 1), c22 = M(1, 0) * M(3, 1) - M(3, 0) * M(1, 1), c23 = M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1);
    float f0[4] = {c00, c00, c02, c03}, f1[4] = {c04, c04, c06, c07}, f2[4] = {c08, c08, c10, c11};
    float f3[4] = {c12, c12, c14, c15}, f4[4] = {c16, c16, c18, c19}, f5[4] = {c20, c20, c22, c23};
    float v0[4] = {M(1, 0), M(0, 0), M(0, 0), M(0, 0)}, v1[4] = {M(1, 1), M(0, 1), M(0, 1), M(0, 1)};
    float v2[4] = {M(1, 2), M(0, 2), M(0, 2), M(0, 2)}, v3[4] = {M(1, 3), M(0, 3), M(0, 3), M(0, 3)};
    Mat4 inv;
    for (int i = 0; i < 4; ++i) {
        float sa = (i & 1) ? -1.0f : 1.0f, sb = -sa;
        inv.m[0 + i] = ((v1[i] * f0[i] - v2[i] * f1[i]) + v3[i] * f2[i]) * sa;
        inv.m[4 + i] = ((v0[i] * f0[i] - v2[i] * f3[i]) + v3[i] * f4[i]) * sb;
        inv.m[8 + i] = ((v0[i] * f1[i] - v1[i] * f3[i]) + v3[i] * f5[i]) * sa;
        inv.m[12 + i] = ((v0[i] * f2[i] - v1[i] * f4[i]) + v2[i] * f5[i]) * sb;
    }
    float det = ((M(0, 0) * inv.m[0] + M(0, 1) * inv.m[4]) + M(0, 2) * inv.m[8]) + M(0, 3) * inv.m[12];
    float rcp = 1.0f / det;
    for (float& x : inv.m) x *= rcp;
    return inv;
}
static void xform_vec3(const Mat4& t, float x, float y, float z, float out[3]) {   // glam transform_vector3
    for (int i = 0; i < 3; ++i) out[i] = (t.m[i] * x + t.m[4 + i] * y) + t.m[8 + i] * z;
}
static void v3_normalize_glam(float v[3]) {   // Vec3::normalize = v * (1 / length)
    float r = 1.0f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] *= r; v[1] *= r; v[2] *= r;
}

// ---------------------------------------------------------------------------------------------- geometry.rs
namespace geometry {

void encode_octahedral_normal(const float n[3], float out[2]) {   // geometry.rs:56-76 (frt_vertex_normal.hpp: the same function runs on the device)
    const f2 e = encode_vertex_normal(mk3(n[0], n[1], n[2]));
    out[0] = e.x; out[1] = e.y;
}

static void push_vertex(Geometry& g, float x, float y, float z, const float nrm[3], float u, float v, const float tan[4]) {
    g.positions.insert(g.positions.end(), {x, y, z, 1.0f});
    frt_vertex_attr a;
    encode_octahedral_normal(nrm, a.normal);
    a.uv[0] = u; a.uv[1] = v;
    memcpy(a.tangent, tan, 16);
    g.attributes.push_back(a);
}

Geometry create_plane() {   // geometry.rs:79-117: unit XZ quad, normal +Y
    Geometry g;
    const float up[3] = {0, 1, 0}, tan[4] = {1, 0, 0, 1};
    const float P[4][5] = {{-0.5f, 0.5f, 0, 1}, {0.5f, 0.5f, 1, 1}, {-0.5f, -0.5f, 0, 0}, {0.5f, -0.5f, 1, 0}};   // x, z, u, v
    for (auto& p : P) push_vertex(g, p[0], 0.0f, p[1], up, p[2], p[3], tan);
    g.indices = {0, 1, 2, 2, 1, 3};
    return g;
}

Geometry create_cube() {   // geometry.rs:120-219: 6 faces x 4 vertices, per-face normal + tangent
    struct Face { float n[3]; float t[4]; float c[4][3]; };
    const float h = 0.5f;
    const Face faces[6] = {
        {{0, 0, 1}, {1, 0, 0, 1}, {{-h, -h, h}, {h, -h, h}, {h, h, h}, {-h, h, h}}},        // front
        {{0, 0, -1}, {-1, 0, 0, 1}, {{h, -h, -h}, {-h, -h, -h}, {-h, h, -h}, {h, h, -h}}},  // back
        {{0, 1, 0}, {1, 0, 0, 1}, {{-h, h, h}, {h, h, h}, {h, h, -h}, {-h, h, -h}}},        // top
        {{0, -1, 0}, {1, 0, 0, 1}, {{-h, -h, -h}, {h, -h, -h}, {h, -h, h}, {-h, -h, h}}},   // bottom
        {{1, 0, 0}, {0, 0, -1, 1}, {{h, -h, h}, {h, -h, -h}, {h, h, -h}, {h, h, h}}},       // right
        {{-1, 0, 0}, {0, 0, 1, 1}, {{-h, -h, -h}, {-h, -h, h}, {-h, h, h}, {-h, h, -h}}},   // left
    };
    const float uv[4][2] = {{0, 1}, {1, 1}, {1, 0}, {0, 0}};
    Geometry g;
    for (uint32_t f = 0; f < 6; ++f) {
        for (int k = 0; k < 4; ++k) push_vertex(g, faces[f].c[k][0], faces[f].c[k][1], faces[f].c[k][2], faces[f].n, uv[k][0], uv[k][1], faces[f].t);
        uint32_t b = 4 * f;
        g.indices.insert(g.indices.end(), {b, b + 1, b + 2, b, b + 2, b + 3});
    }
    return g;
}

Geometry create_sphere(uint32_t subdivisions) {   // geometry.rs:222-346: icosphere, radius 0.5, midpoint cache
    Geometry g;
    const float tan[4] = {1, 0, 0, 1};
    auto add_unit = [&](float x, float y, float z) -> uint32_t {
        float len = sqrtf(x * x + y * y + z * z);
        float n[3] = {x / len, y / len, z / len};
        push_vertex(g, n[0] * 0.5f, n[1] * 0.5f, n[2] * 0.5f, n, 0.0f, 0.0f, tan);
        return (uint32_t)g.attributes.size() - 1u;
    };
    const float t = (1.0f + sqrtf(5.0f)) / 2.0f;
    const float seed[12][3] = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t},
                               {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
    for (auto& s : seed) add_unit(s[0], s[1], s[2]);
    std::vector<uint32_t> faces = {0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
                                   3, 9, 4, 3, 4, 2, 3, 2, 6, 3, 6, 8, 3, 8, 9, 4, 9, 5, 2, 4, 11, 6, 2, 10, 8, 6, 7, 9, 8, 1};
    std::map<uint64_t, uint32_t> cache;   // geometry.rs:282 — point lookups only, so ordering of the map is irrelevant
    auto midpoint = [&](uint32_t a, uint32_t b) -> uint32_t {
        uint64_t key = a < b ? ((uint64_t)a << 32 | b) : ((uint64_t)b << 32 | a);
        auto it = cache.find(key);
        if (it != cache.end()) return it->second;
        const float* pa = &g.positions[4 * a];
        const float* pb = &g.positions[4 * b];
        float mx = (pa[0] + pb[0]) * 0.5f, my = (pa[1] + pb[1]) * 0.5f, mz = (pa[2] + pb[2]) * 0.5f;
        uint32_t id = add_unit(mx, my, mz);
        cache.emplace(key, id);
        return id;
    };
    for (uint32_t level = 0; level < subdivisions; ++level) {
        std::vector<uint32_t> next;
        next.reserve(faces.size() * 4);
        for (size_t f = 0; f < faces.size(); f += 3) {
            uint32_t v1 = faces[f], v2 = faces[f + 1], v3 = faces[f + 2];
            uint32_t a = midpoint(v1, v2), b = midpoint(v2, v3), c = midpoint(v3, v1);
            next.insert(next.end(), {v1, a, c, v2, b, a, v3, c, b, a, b, c});
        }
        faces.swap(next);
    }
    g.indices = faces;
    return g;
}

Geometry create_crystal() {   // geometry.rs:350-434: 16 flat faces, unshared vertices
    Geometry g;
    const float tan[4] = {1, 0, 0, 1};
    const float top[3] = {0, 1, 0}, bottom[3] = {0, -1, 0};
    const float ring[4][2] = {{0.3f, 0.3f}, {-0.3f, 0.3f}, {-0.3f, -0.3f}, {0.3f, -0.3f}};   // x, z
    auto ringp = [&](int i, float y, float out[3]) { out[0] = ring[i & 3][0]; out[1] = y; out[2] = ring[i & 3][1]; };
    auto face = [&](const float p0[3], const float p1[3], const float p2[3]) {
        float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        v3_normalize_glam(n);
        uint32_t base = (uint32_t)g.attributes.size();
        push_vertex(g, p0[0], p0[1], p0[2], n, 0, 0, tan);
        push_vertex(g, p1[0], p1[1], p1[2], n, 0, 0, tan);
        push_vertex(g, p2[0], p2[1], p2[2], n, 0, 0, tan);
        g.indices.insert(g.indices.end(), {base, base + 1, base + 2});
    };
    float a[3], b[3], c[3], d[3];
    for (int i = 0; i < 4; ++i) { ringp(i + 1, 0.5f, a); ringp(i, 0.5f, b); face(top, a, b); }
    for (int i = 0; i < 4; ++i) {
        ringp(i, 0.5f, a); ringp(i + 1, 0.5f, b); ringp(i + 1, -0.5f, c); ringp(i, -0.5f, d);
        face(a, b, c);
        face(a, c, d);
    }
    for (int i = 0; i < 4; ++i) { ringp(i, -0.5f, a); ringp(i + 1, -0.5f, b); face(bottom, a, b); }
    return g;
}

} // namespace geometry

// ---------------------------------------------------------------------------------------------- material.rs
MaterialBuilder::MaterialBuilder(float r, float g, float b, float a) {
    memset(&m, 0, sizeof(m));
    m.base_color[0] = r; m.base_color[1] = g; m.base_color[2] = b; m.base_color[3] = a;
    m.roughness = 0.5f; m.ior = 1.0f; m.light_index = -1;
    m.tex_info_0 = m.tex_info_1 = m.tex_info_2 = 0xFFFFFFFFu;
}

// ---------------------------------------------------------------------------------------------- builder.rs
static const size_t kTexBytes = kTextureLayerBytes;

static std::vector<uint8_t> make_texture(uint8_t (*fn)(uint32_t, uint32_t, int)) {
    std::vector<uint8_t> t(kTexBytes);
    for (uint32_t y = 0; y < 1024; ++y)
        for (uint32_t x = 0; x < 1024; ++x)
            for (int ch = 0; ch < 4; ++ch) t[(y * 1024u + x) * 4u + ch] = fn(x, y, ch);
    return t;
}

SceneBuilder::SceneBuilder() {
    // builder.rs:41-91 — colour {white, 64-px checker, black}; data {white, flat normal, black}
    color_textures.push_back(make_texture([](uint32_t, uint32_t, int) -> uint8_t { return 255; }));
    color_textures.push_back(make_texture([](uint32_t x, uint32_t y, int ch) -> uint8_t {
        if (ch == 3) return 255;
        return (((x / 64) + (y / 64)) % 2 == 0) ? 255 : 0;
    }));
    color_textures.push_back(make_texture([](uint32_t, uint32_t, int ch) -> uint8_t { return ch == 3 ? 255 : 0; }));
    data_textures.push_back(color_textures[0]);
    data_textures.push_back(make_texture([](uint32_t, uint32_t, int ch) -> uint8_t { return ch < 2 ? 128 : 255; }));
    data_textures.push_back(color_textures[2]);
    for (int i = 0; i < 256; ++i) {   // Rgba8UnormSrgb decode (builder.rs:489), IEC 61966-2-1
        double c = i / 255.0;
        srgb_lut[i] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
    }
}

uint32_t SceneBuilder::add_color_texture(const uint8_t* p) { color_textures.emplace_back(p, p + kTexBytes); return (uint32_t)color_textures.size() - 1; }
uint32_t SceneBuilder::add_data_texture(const uint8_t* p) { data_textures.emplace_back(p, p + kTexBytes); return (uint32_t)data_textures.size() - 1; }
uint32_t SceneBuilder::add_material(const frt_material& m) { materials.push_back(m); return (uint32_t)materials.size() - 1; }
uint32_t SceneBuilder::add_light(const frt_light& l) { lights.push_back(l); return (uint32_t)lights.size() - 1; }

uint32_t SceneBuilder::add_mesh(const Geometry& g) {
    MeshInfo mi = {(uint32_t)attributes.size(), (uint32_t)indices.size(), {0, 0}};
    attributes.insert(attributes.end(), g.attributes.begin(), g.attributes.end());
    indices.insert(indices.end(), g.indices.begin(), g.indices.end());
    mesh_infos.push_back(mi);
    mesh_positions.push_back(g.positions);
    mesh_index_counts.push_back((uint32_t)g.indices.size());
    return (uint32_t)mesh_infos.size() - 1;
}

void SceneBuilder::add_instance(uint32_t mesh_id, uint32_t mat_id, const Mat4& t) {
    InstanceRec r{};
    r.mesh_id = mesh_id; r.mat_id = mat_id;
    memcpy(r.m, t.m, sizeof(r.m));
    instances.push_back(r);
    built = false;
}

static frt_light make_quad_light(const float pos[3], const float u[3], const float v[3], const float emission[4]) {
    float cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
    frt_light l{};
    memcpy(l.position, pos, 12); memcpy(l.u, u, 12); memcpy(l.v, v, 12); memcpy(l.emission, emission, 16);
    l.type_ = 0;
    l.area = sqrtf(cx * cx + cy * cy + cz * cz) * 4.0f;   // |(2u) x (2v)|
    return l;
}
static frt_light make_sphere_light(const float center[3], float radius, const float emission[4]) {
    frt_light l{};
    memcpy(l.position, center, 12); memcpy(l.emission, emission, 16);
    l.type_ = 1;
    l.area = 4.0f * 3.14159265358979323846f * radius * radius;
    l.v[0] = radius;
    return l;
}
void SceneBuilder::add_quad_light(const float pos[3], const float u[3], const float v[3], const float emission[4]) { lights.push_back(make_quad_light(pos, u, v, emission)); }
void SceneBuilder::add_sphere_light(const float center[3], float radius, const float emission[4]) { lights.push_back(make_sphere_light(center, radius, emission)); }
frt_light quad_light_record(const Mat4& t, const float emission[4]) {
    float u[3], v[3];
    xform_vec3(t, 1, 0, 0, u); xform_vec3(t, 0, 0, -1, v);
    for (int i = 0; i < 3; ++i) { u[i] *= 0.5f; v[i] *= 0.5f; }
    return make_quad_light(&t.m[12], u, v, emission);
}
frt_light sphere_light_record(const Mat4& t, const float emission[4]) {
    float x[3];
    xform_vec3(t, 1, 0, 0, x);
    float scale = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    return make_sphere_light(&t.m[12], scale * 0.5f, emission);
}
void light_emissive_factor(const float color[3], float intensity, float out[3]) {
    for (int k = 0; k < 3; ++k) out[k] = color[k] * intensity;
}
frt_material light_emissive_material(size_t light_index, const float color[3], float intensity) {
    float e[3];
    light_emissive_factor(color, intensity, e);
    return MaterialBuilder(1, 1, 1, 1).light_index((int32_t)light_index).emissive_factor(e[0], e[1], e[2]).texture(0);
}
void SceneBuilder::register_quad_light(uint32_t mesh_id, const Mat4& t, const float color[3], float intensity) {
    uint32_t mat = add_material(light_emissive_material(lights.size(), color, intensity));
    add_instance(mesh_id, mat, t);
    instances.back().light = (int32_t)lights.size(); instances.back().light_kind = 0;
    const float em[4] = {color[0], color[1], color[2], intensity};
    lights.push_back(quad_light_record(t, em));
}
void SceneBuilder::register_sphere_light(uint32_t mesh_id, const Mat4& t, const float color[3], float intensity) {
    uint32_t mat = add_material(light_emissive_material(lights.size(), color, intensity));
    add_instance(mesh_id, mat, t);
    instances.back().light = (int32_t)lights.size(); instances.back().light_kind = 1;
    const float em[4] = {color[0], color[1], color[2], intensity};
    lights.push_back(sphere_light_record(t, em));
}

// Instances -> world-space triangles (contract): p_world = ((c0*x + c1*y) + c2*z) + c3 in f32,
// e1 = v1 - v0, e2 = v2 - v0; world_to_object 3x3 by cofactors in double, rounded once to f32.
static double cofactor_inverse(const float m[16], float w2o[9], uint32_t& flip) {
    double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
    double k00 = e * i - f * h, k01 = f * g - d * i, k02 = d * h - e * g;
    double det = a * k00 + b * k01 + c * k02;
    double inv[3][3] = {{k00 / det, (c * h - b * i) / det, (b * f - c * e) / det},
                        {k01 / det, (a * i - c * g) / det, (c * d - a * f) / det},
                        {k02 / det, (b * g - a * h) / det, (a * e - b * d) / det}};
    for (int col = 0; col < 3; ++col) for (int row = 0; row < 3; ++row) w2o[3 * col + row] = (float)inv[row][col];
    flip = det < 0.0 ? 1u : 0u;
    return det;
}
bool instance_inverse(const float m[16], float w2o[9], uint32_t& flip) {
    for (int k = 0; k < 16; ++k) if (!std::isfinite(m[k])) return false;
    float w[9]; uint32_t fl;
    if (!(cofactor_inverse(m, w, fl) != 0.0)) return false;
    memcpy(w2o, w, sizeof(w)); flip = fl;
    return true;
}
void world_triangle(const float m[16], const float* P, const uint32_t idx[3], TriRec& t) {
    float w[3][3];
    for (int k = 0; k < 3; ++k) {
        float x = P[4 * idx[k]], y = P[4 * idx[k] + 1], z = P[4 * idx[k] + 2];
        for (int r = 0; r < 3; ++r) w[k][r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r];
    }
    for (int r = 0; r < 3; ++r) { t.v0[r] = w[0][r]; t.e1[r] = w[1][r] - w[0][r]; t.e2[r] = w[2][r] - w[0][r]; }
}
void SceneBuilder::flatten() {
    tris.clear(); tri_instance.clear();
    for (size_t ii = 0; ii < instances.size(); ++ii) {
        InstanceRec& in = instances[ii];
        cofactor_inverse(in.m, in.w2o, in.flip);
        in.first_tri = (uint32_t)tris.size();
        const std::vector<float>& P = mesh_positions[in.mesh_id];
        const uint32_t* idx = &indices[mesh_infos[in.mesh_id].index_offset];
        uint32_t nidx = mesh_index_counts[in.mesh_id];
        for (uint32_t k = 0; k + 2 < nidx; k += 3) {
            TriRec t;
            world_triangle(in.m, P.data(), idx + k, t);
            tris.push_back(t);
            tri_instance.push_back((uint32_t)ii);
        }
        in.tri_count = (uint32_t)tris.size() - in.first_tri;
    }
}

std::string check_instance_transforms(uint32_t n, const uint32_t* ids, const float* mats, size_t num_instances) {
    if (n > 0 && (!ids || !mats)) return "null ids or matrices";
    for (uint32_t k = 0; k < n; ++k) {
        if (ids[k] >= num_instances) return "instance id " + std::to_string(ids[k]) + " out of range (" + std::to_string(num_instances) + " instances)";
        float w2o[9]; uint32_t flip;
        if (!instance_inverse(mats + 16 * (size_t)k, w2o, flip))
            return "matrix " + std::to_string(k) + " (instance " + std::to_string(ids[k]) + ") has a non-finite entry or a singular 3x3";
    }
    return "";
}

int SceneBuilder::set_instance_transforms(uint32_t n, const uint32_t* ids, const float* mats) {
    if (!built) { error = "set_instance_transforms: scene is not built"; return FRT_ERR_STATE; }
    const std::string bad = check_instance_transforms(n, ids, mats, instances.size());
    if (!bad.empty()) { error = "set_instance_transforms: " + bad; return FRT_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < n; ++k) {      // in order: an id given twice ends with its last matrix
        InstanceRec& in = instances[ids[k]];
        memcpy(in.m, mats + 16 * (size_t)k, sizeof(in.m));
        instance_inverse(in.m, in.w2o, in.flip);
        instances_dev[ids[k]].flip = in.flip;
        memcpy(instances_dev[ids[k]].w2o, in.w2o, sizeof(in.w2o));
        const float* P = mesh_positions[in.mesh_id].data();
        const uint32_t* idx = &indices[mesh_infos[in.mesh_id].index_offset];
        for (uint32_t j = 0; j < in.tri_count; ++j) {
            const uint32_t id = in.first_tri + j;
            TriRec& t = tris[id];
            world_triangle(in.m, P, idx + 3 * j, t);
            TriSlot& o = tri_slots[tri_slot_of[id]];      // same slot, id and instance bits
            for (int r = 0; r < 3; ++r) { o.q[r] = t.v0[r]; o.q[4 + r] = t.e1[r]; o.q[8 + r] = t.e2[r]; }
        }
        if (in.light >= 0) {
            Mat4 t; memcpy(t.m, in.m, sizeof(t.m));
            frt_light& l = lights[(size_t)in.light];
            float em[4]; memcpy(em, l.emission, sizeof(em));
            l = in.light_kind == 0 ? quad_light_record(t, em) : sphere_light_record(t, em);
        }
    }
    refit();
    return FRT_OK;
}

std::string check_mesh_vertices(const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts, uint32_t mesh_nverts) {
    if (!pos4) return "null positions";
    if (nverts != mesh_nverts) return std::to_string(nverts) + " vertices given, the mesh has " + std::to_string(mesh_nverts) + " (the topology is fixed)";
    for (size_t k = 0; k < (size_t)nverts * 4; ++k) if (!std::isfinite(pos4[k])) return "position of vertex " + std::to_string(k / 4) + " is not finite";
    if (attrs) {
        const float* a = reinterpret_cast<const float*>(attrs);
        for (size_t k = 0; k < (size_t)nverts * 8; ++k) if (!std::isfinite(a[k])) return "attributes of vertex " + std::to_string(k / 8) + " are not finite";
    }
    return "";
}

void build_vertex_corners(const uint32_t* idx, uint32_t nidx, uint32_t nverts, std::vector<uint32_t>& offsets, std::vector<uint32_t>& corners) {
    offsets.assign((size_t)nverts + 1u, 0u);
    corners.assign(nidx, 0u);
    for (uint32_t c = 0; c < nidx; ++c) if (idx[c] < nverts) ++offsets[(size_t)idx[c] + 1u];
    for (uint32_t v = 0; v < nverts; ++v) offsets[(size_t)v + 1u] += offsets[v];
    std::vector<uint32_t> next(offsets.begin(), offsets.end() - 1);
    for (uint32_t c = 0; c < nidx; ++c) if (idx[c] < nverts) corners[next[idx[c]]++] = c;      // ascending c per vertex: a counting sort is stable
}

// What each call of the mesh-edit family checks first, in this order: the scene is built, no FRT_DEFORM_DEVICE (`renderer_call`: the call that takes it),
// no unknown flag bit, the mesh id. A call without flags passes 0.
int SceneBuilder::check_mesh_call(const char* call, const char* renderer_call, uint32_t mesh_id, uint32_t flags) {
    const std::string c(call);
    if (!built) { error = c + ": scene is not built"; return FRT_ERR_STATE; }
    if (flags & FRT_DEFORM_DEVICE) { error = c + ": FRT_DEFORM_DEVICE is for " + renderer_call + " only (a scene lives in host memory)"; return FRT_ERR_INVALID_ARG; }
    if (flags & ~FRT_DEFORM_RECOMPUTE_NORMALS) { error = c + ": unknown flag bits"; return FRT_ERR_INVALID_ARG; }
    if (mesh_id >= mesh_positions.size()) { error = c + ": mesh id " + std::to_string(mesh_id) + " out of range (" + std::to_string(mesh_positions.size()) + " meshes)"; return FRT_ERR_INVALID_ARG; }
    return FRT_OK;
}
int SceneBuilder::set_mesh_vertices(uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts, uint32_t flags) {
    if (const int rc = check_mesh_call("set_mesh_vertices", "frt_renderer_set_mesh_vertices_ex", mesh_id, flags)) return rc;
    const std::string bad = check_mesh_vertices(pos4, attrs, nverts, (uint32_t)(mesh_positions[mesh_id].size() / 4));
    if (!bad.empty()) { error = "set_mesh_vertices: " + bad; return FRT_ERR_INVALID_ARG; }
    const bool recompute = (flags & FRT_DEFORM_RECOMPUTE_NORMALS) != 0;
    mesh_positions[mesh_id].assign(pos4, pos4 + (size_t)nverts * 4);
    if (attrs) std::copy(attrs, attrs + nverts, attributes.begin() + mesh_infos[mesh_id].vertex_offset);
    const float* P = mesh_positions[mesh_id].data();
    const uint32_t* idx = &indices[mesh_infos[mesh_id].index_offset];
    if (recompute) {      // after the attributes of the call: uv and tangent are the caller's, the normal is the mesh's (a vertex that keeps its normal keeps the caller's)
        struct P4 { float x, y, z, w; };
        const uint32_t nidx = mesh_index_counts[mesh_id];
        std::vector<uint32_t> off, corners;
        build_vertex_corners(idx, nidx, nverts, off, corners);
        for (uint32_t v = 0; v < nverts; ++v) {
            f2 e;
            if (!recomputed_vertex_normal(corners.data(), off[v], off[v + 1u], idx, nidx, reinterpret_cast<const P4*>(P), nverts, e)) continue;
            frt_vertex_attr& a = attributes[(size_t)mesh_infos[mesh_id].vertex_offset + v];
            a.normal[0] = e.x; a.normal[1] = e.y;
        }
    }
    for (InstanceRec& in : instances) {      // in instance order, under each instance's current matrix
        if (in.mesh_id != mesh_id) continue;
        for (uint32_t j = 0; j < in.tri_count; ++j) {
            const uint32_t id = in.first_tri + j;
            TriRec& t = tris[id];
            world_triangle(in.m, P, idx + 3 * j, t);
            TriSlot& o = tri_slots[tri_slot_of[id]];      // same slot, id and instance bits
            for (int r = 0; r < 3; ++r) { o.q[r] = t.v0[r]; o.q[4 + r] = t.e1[r]; o.q[8 + r] = t.e2[r]; }
            if (attrs || recompute) write_shade_tri(id);
        }
    }
    refit();
    return FRT_OK;
}

// ---------------------------------------------------------------------------------------------- skinning ("Skinning")
std::string check_mesh_skin(const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints, uint32_t mesh_nverts) {
    if (!joints4 || !weights4) return "null joints or weights";
    if (nverts != mesh_nverts) return std::to_string(nverts) + " vertices given, the mesh has " + std::to_string(mesh_nverts);
    if (njoints == 0 || njoints > 0x10000u) return std::to_string(njoints) + " joints (1 to 65536: a joint index is 16 bits)";
    for (size_t k = 0; k < (size_t)nverts * 4; ++k) {
        if (joints4[k] >= njoints) return "vertex " + std::to_string(k / 4) + " names joint " + std::to_string(joints4[k]) + " of " + std::to_string(njoints);
        if (!std::isfinite(weights4[k]) || weights4[k] < 0.0f) return "a weight of vertex " + std::to_string(k / 4) + " is negative or not finite";
    }
    return "";
}
std::string check_mesh_pose(const float* joint_mats, uint32_t njoints, uint32_t bound_joints, bool host_memory) {
    if (bound_joints == 0) return "the mesh has no skin (set_mesh_skin)";
    if (njoints != bound_joints) return std::to_string(njoints) + " joint matrices given, the skin was bound with " + std::to_string(bound_joints);
    if (!joint_mats) return "null joint matrices";
    for (size_t k = 0; host_memory && k < (size_t)njoints * 16; ++k) if (!std::isfinite(joint_mats[k])) return "joint matrix " + std::to_string(k / 16) + " has a non-finite entry";
    return "";
}
int SceneBuilder::set_mesh_skin(uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints, uint32_t skin_flags) {
    if (const int rc = check_mesh_call("set_mesh_skin", "", mesh_id, 0u)) return rc;
    if (skin_flags & ~FRT_SKIN_DUAL_QUATERNION) { error = "set_mesh_skin: unknown flag bits"; return FRT_ERR_INVALID_ARG; }
    if (!joints4) {
        if (mesh_id < mesh_skins.size()) mesh_skins[mesh_id] = MeshSkin();
        return FRT_OK;
    }
    const std::string bad = check_mesh_skin(joints4, weights4, nverts, njoints, (uint32_t)(mesh_positions[mesh_id].size() / 4));
    if (!bad.empty()) { error = "set_mesh_skin: " + bad; return FRT_ERR_INVALID_ARG; }
    if (mesh_skins.size() <= mesh_id) mesh_skins.resize((size_t)mesh_id + 1u);
    MeshSkin& k = mesh_skins[mesh_id];
    k.njoints = njoints; k.mode = skin_flags;
    k.joints.assign(joints4, joints4 + (size_t)nverts * 4);
    k.weights.assign(weights4, weights4 + (size_t)nverts * 4);
    k.bind = mesh_positions[mesh_id];
    return FRT_OK;
}
int SceneBuilder::set_mesh_pose(uint32_t mesh_id, const float* joint_mats, uint32_t njoints, uint32_t flags) {
    return set_mesh_pose_ex(mesh_id, joint_mats, njoints, nullptr, 0u, flags);
}

// ---------------------------------------------------------------------------------------------- morph targets ("Morph targets")
std::string check_mesh_morph_targets(const float* deltas3, uint32_t nverts, uint32_t ntargets, uint32_t mesh_nverts) {
    if (!deltas3) return "null deltas";
    if (nverts != mesh_nverts) return std::to_string(nverts) + " vertices given, the mesh has " + std::to_string(mesh_nverts);
    if (ntargets == 0 || ntargets > FRT_MAX_MORPH_TARGETS) return std::to_string(ntargets) + " targets (1 to " + std::to_string(FRT_MAX_MORPH_TARGETS) + ")";
    for (size_t k = 0; k < (size_t)ntargets * nverts * 3; ++k)
        if (!std::isfinite(deltas3[k])) return "a delta of target " + std::to_string(k / 3 / nverts) + ", vertex " + std::to_string(k / 3 % nverts) + " is not finite";
    return "";
}
std::string check_mesh_morph_weights(const float* weights, uint32_t ntargets, uint32_t bound_targets, bool host_memory) {
    if (bound_targets == 0) return "the mesh has no morph targets (set_mesh_morph_targets)";
    if (ntargets != bound_targets) return std::to_string(ntargets) + " weights given, " + std::to_string(bound_targets) + " targets are bound";
    if (!weights) return "null weights";
    for (uint32_t t = 0; host_memory && t < ntargets; ++t) if (!std::isfinite(weights[t])) return "the weight of target " + std::to_string(t) + " is not finite";
    return "";
}
int SceneBuilder::set_mesh_morph_targets(uint32_t mesh_id, const float* deltas3, uint32_t nverts, uint32_t ntargets) {
    if (const int rc = check_mesh_call("set_mesh_morph_targets", "", mesh_id, 0u)) return rc;
    if (!deltas3) {
        if (mesh_id < mesh_morphs.size()) mesh_morphs[mesh_id] = MeshMorph();
        return FRT_OK;
    }
    const std::string bad = check_mesh_morph_targets(deltas3, nverts, ntargets, (uint32_t)(mesh_positions[mesh_id].size() / 4));
    if (!bad.empty()) { error = "set_mesh_morph_targets: " + bad; return FRT_ERR_INVALID_ARG; }
    if (mesh_morphs.size() <= mesh_id) mesh_morphs.resize((size_t)mesh_id + 1u);
    MeshMorph& k = mesh_morphs[mesh_id];
    k.ntargets = ntargets;
    k.deltas.assign(deltas3, deltas3 + (size_t)ntargets * nverts * 3);
    k.base = mesh_positions[mesh_id];
    return FRT_OK;
}
// The morphed positions of mesh `mesh_id` under checked weights; "" or what is wrong with them.
static std::string morph_mesh(const SceneBuilder::MeshMorph& k, const float* weights, std::vector<float>& morphed) {
    const size_t nverts = k.base.size() / 4;
    morphed.resize(k.base.size());
    for (size_t v = 0; v < nverts; ++v) morphed_position(&k.base[4 * v], &k.deltas[3 * v], 3 * nverts, weights, k.ntargets, &morphed[4 * v]);
    for (size_t c = 0; c < morphed.size(); ++c)
        if (!std::isfinite(morphed[c])) return "the morphed position of vertex " + std::to_string(c / 4) + " is not finite";
    return "";
}
int SceneBuilder::set_mesh_morph_weights(uint32_t mesh_id, const float* weights, uint32_t ntargets, uint32_t flags) {
    if (const int rc = check_mesh_call("set_mesh_morph_weights", "frt_renderer_set_mesh_morph_weights", mesh_id, flags)) return rc;
    std::string bad = check_mesh_morph_weights(weights, ntargets, mesh_id < mesh_morphs.size() ? mesh_morphs[mesh_id].ntargets : 0u);
    std::vector<float> morphed;
    if (bad.empty()) bad = morph_mesh(mesh_morphs[mesh_id], weights, morphed);
    if (!bad.empty()) { error = "set_mesh_morph_weights: " + bad; return FRT_ERR_INVALID_ARG; }
    return set_mesh_vertices(mesh_id, morphed.data(), nullptr, (uint32_t)(morphed.size() / 4), flags);
}
// The skinned positions of `bind` under a checked palette; "" or what is wrong with them.
static std::string skin_mesh(const SceneBuilder::MeshSkin& k, const std::vector<float>& bind, const float* joint_mats, std::vector<float>& skinned) {
    const uint32_t nverts = (uint32_t)(bind.size() / 4);
    skinned.resize(bind.size());
    for (uint32_t v = 0; v < nverts; ++v) {
        if (k.mode == FRT_SKIN_DUAL_QUATERNION) {      // each of the vertex's joints converted where it is named, as the kernel's lane converts it
            SkinDualQuat dq[4];
            for (int s = 0; s < 4; ++s) dq[s] = skin_dq_of_joint(joint_mats + 16 * (size_t)k.joints[4 * (size_t)v + s]);
            skinned_position_dq(&bind[4 * (size_t)v], dq, &k.weights[4 * (size_t)v], &skinned[4 * (size_t)v]);
            continue;
        }
        float m[4][16];
        for (int s = 0; s < 4; ++s) memcpy(m[s], joint_mats + 16 * (size_t)k.joints[4 * (size_t)v + s], sizeof(m[s]));
        skinned_position(&bind[4 * (size_t)v], m, &k.weights[4 * (size_t)v], &skinned[4 * (size_t)v]);
    }
    for (size_t c = 0; c < skinned.size(); ++c)
        if (!std::isfinite(skinned[c])) return "the skinned position of vertex " + std::to_string(c / 4) + " is not finite";
    return "";
}
// set_mesh_pose's checks in set_mesh_pose's order; with morph weights the morph's follow, and the morphed positions stand where the bind pose stood.
// `posed`: the positions the call would apply. "" or what refuses the call.
std::string SceneBuilder::pose_mesh(uint32_t mesh_id, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, bool check_inputs, std::vector<float>& posed) const {
    std::string bad = check_mesh_pose(joint_mats, njoints, mesh_id < mesh_skins.size() ? mesh_skins[mesh_id].njoints : 0u, check_inputs);
    if (!bad.empty()) return bad;
    std::vector<float> morphed;
    if (morph_weights || ntargets) {
        bad = check_mesh_morph_weights(morph_weights, ntargets, mesh_id < mesh_morphs.size() ? mesh_morphs[mesh_id].ntargets : 0u, check_inputs);
        if (bad.empty()) bad = morph_mesh(mesh_morphs[mesh_id], morph_weights, morphed);
        if (!bad.empty()) return bad;
    }
    const MeshSkin& k = mesh_skins[mesh_id];
    return skin_mesh(k, morphed.empty() ? k.bind : morphed, joint_mats, posed);
}
int SceneBuilder::set_mesh_pose_ex(uint32_t mesh_id, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags) {
    if (const int rc = check_mesh_call("set_mesh_pose", "frt_renderer_set_mesh_pose", mesh_id, flags)) return rc;
    std::vector<float> skinned;
    const std::string bad = pose_mesh(mesh_id, joint_mats, njoints, morph_weights, ntargets, true, skinned);
    if (!bad.empty()) { error = "set_mesh_pose: " + bad; return FRT_ERR_INVALID_ARG; }
    return set_mesh_vertices(mesh_id, skinned.data(), nullptr, (uint32_t)(skinned.size() / 4), flags);
}

// ---------------------------------------------------------------------------------------------- posing several meshes ("Posing several meshes")
std::string check_pose_batch(uint32_t n, const uint32_t* mesh_ids, size_t num_meshes, bool palette, bool weights) {
    if (n == 0 || n > FRT_MAX_POSE_MESHES) return std::to_string(n) + " meshes (1 to " + std::to_string(FRT_MAX_POSE_MESHES) + ")";
    if (!mesh_ids) return "null mesh ids";
    if (!palette && !weights) return "neither joint matrices nor morph weights given";
    std::vector<uint32_t> sorted(mesh_ids, mesh_ids + n);
    for (uint32_t k = 0; k < n; ++k)
        if (mesh_ids[k] >= num_meshes) return "mesh id " + std::to_string(mesh_ids[k]) + " out of range (" + std::to_string(num_meshes) + " meshes)";
    std::sort(sorted.begin(), sorted.end());
    for (uint32_t k = 1; k < n; ++k) if (sorted[k] == sorted[k - 1]) return "mesh id " + std::to_string(sorted[k]) + " is given twice";
    return "";
}
// Everything is validated first, the posed vertices of every mesh included; then the meshes are applied in the order given, each through
// set_mesh_vertices (whose refit makes the same boxes once or n times: min and max are exact).
int SceneBuilder::set_mesh_poses(uint32_t n, const uint32_t* mesh_ids, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags) {
    if (!built) { error = "set_mesh_poses: scene is not built"; return FRT_ERR_STATE; }
    if (flags & FRT_DEFORM_DEVICE) { error = "set_mesh_poses: FRT_DEFORM_DEVICE is for frt_renderer_set_mesh_poses only (a scene lives in host memory)"; return FRT_ERR_INVALID_ARG; }
    if (flags & ~FRT_DEFORM_RECOMPUTE_NORMALS) { error = "set_mesh_poses: unknown flag bits"; return FRT_ERR_INVALID_ARG; }
    const bool skin = joint_mats || njoints, morph = morph_weights || ntargets;
    std::string bad = check_pose_batch(n, mesh_ids, mesh_positions.size(), skin, morph);
    std::vector<std::vector<float>> posed(bad.empty() ? n : 0u);
    for (uint32_t k = 0; k < n && bad.empty(); ++k) {      // (the palette and the weights are the same for every mesh: their entries are read once)
        const uint32_t m = mesh_ids[k];
        if (skin) bad = pose_mesh(m, joint_mats, njoints, morph_weights, ntargets, k == 0, posed[k]);
        else {
            bad = check_mesh_morph_weights(morph_weights, ntargets, m < mesh_morphs.size() ? mesh_morphs[m].ntargets : 0u, k == 0);
            if (bad.empty()) bad = morph_mesh(mesh_morphs[m], morph_weights, posed[k]);
        }
        if (!bad.empty()) bad = "mesh " + std::to_string(m) + ": " + bad;
    }
    if (!bad.empty()) { error = "set_mesh_poses: " + bad; return FRT_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < n; ++k)
        if (const int rc = set_mesh_vertices(mesh_ids[k], posed[k].data(), nullptr, (uint32_t)(posed[k].size() / 4), flags)) return rc;
    return FRT_OK;
}

// ---------------------------------------------------------------------------------------------- materials, lights, textures
std::string check_material(const frt_material& m, size_t color_layers, size_t data_layers, size_t num_lights) {
    std::string bad;
    const struct { uint32_t id; size_t layers; const char* what; } slots[5] = {
        {m.tex_info_0 & 0xFFFFu, color_layers, "base colour"}, {m.tex_info_0 >> 16, data_layers, "normal"},
        {m.tex_info_1 & 0xFFFFu, data_layers, "occlusion"}, {m.tex_info_1 >> 16, color_layers, "emissive"},
        {m.tex_info_2 & 0xFFFFu, data_layers, "metallic-roughness"}};
    for (const auto& t : slots)
        if (t.id != 0xFFFFu && t.id >= t.layers)
            bad = std::string(t.what) + " texture layer " + std::to_string(t.id) + " does not exist (" + std::to_string(t.layers) + " layers)";
    if (m.light_index >= 0 && (size_t)m.light_index >= num_lights)
        bad = "light_index " + std::to_string(m.light_index) + " does not exist (" + std::to_string(num_lights) + " lights)";
    return bad;
}
std::string check_set_materials(uint32_t n, const uint32_t* ids, const frt_material* mats, size_t num_materials, size_t color_layers, size_t data_layers, size_t num_lights) {
    if (n > 0 && (!ids || !mats)) return "null ids or materials";
    for (uint32_t k = 0; k < n; ++k) {
        if (ids[k] >= num_materials) return "material id " + std::to_string(ids[k]) + " out of range (" + std::to_string(num_materials) + " materials)";
        const std::string bad = check_material(mats[k], color_layers, data_layers, num_lights);
        if (!bad.empty()) return "material " + std::to_string(ids[k]) + ": " + bad;
    }
    return "";
}
std::string check_set_instance_materials(uint32_t n, const uint32_t* iids, const uint32_t* mids, const std::vector<InstanceRec>& instances, size_t num_materials) {
    if (n > 0 && (!iids || !mids)) return "null instance or material ids";
    for (uint32_t k = 0; k < n; ++k) {
        if (iids[k] >= instances.size()) return "instance id " + std::to_string(iids[k]) + " out of range (" + std::to_string(instances.size()) + " instances)";
        if (mids[k] >= num_materials) return "material id " + std::to_string(mids[k]) + " out of range (" + std::to_string(num_materials) + " materials)";
        if (instances[iids[k]].light >= 0)
            return "instance " + std::to_string(iids[k]) + " was registered with light " + std::to_string(instances[iids[k]].light) + ": its material carries the light link (set_light_emission edits it)";
    }
    return "";
}
std::string check_set_texture(int kind, uint32_t layer, const uint8_t* rgba8, size_t color_layers, size_t data_layers) {
    if (kind != 0 && kind != 1) return "kind must be 0 (colour) or 1 (data)";
    if (!rgba8) return "null pixels";
    const size_t layers = kind == 0 ? color_layers : data_layers;
    if (layer >= layers) return std::string(kind == 0 ? "colour" : "data") + " layer " + std::to_string(layer) + " does not exist (" + std::to_string(layers) + " layers)";
    return "";
}
int light_instance(const std::vector<InstanceRec>& instances, uint32_t light) {
    for (size_t i = 0; i < instances.size(); ++i) if (instances[i].light >= 0 && (uint32_t)instances[i].light == light) return (int)i;
    return -1;
}

int SceneBuilder::set_materials(uint32_t n, const uint32_t* ids, const frt_material* mats) {
    if (!built) { error = "set_materials: scene is not built"; return FRT_ERR_STATE; }
    const std::string bad = check_set_materials(n, ids, mats, materials.size(), color_textures.size(), data_textures.size(), lights.size());
    if (!bad.empty()) { error = "set_materials: " + bad; return FRT_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < n; ++k) materials[ids[k]] = mats[k];      // in order: an id given twice ends with its last value
    return FRT_OK;
}
int SceneBuilder::set_instance_materials(uint32_t n, const uint32_t* iids, const uint32_t* mids) {
    if (!built) { error = "set_instance_materials: scene is not built"; return FRT_ERR_STATE; }
    const std::string bad = check_set_instance_materials(n, iids, mids, instances, materials.size());
    if (!bad.empty()) { error = "set_instance_materials: " + bad; return FRT_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < n; ++k) {      // in order, as above
        InstanceRec& in = instances[iids[k]];
        in.mat_id = mids[k];
        instances_dev[iids[k]].mat_id = mids[k];
        for (uint32_t j = 0; j < in.tri_count; ++j) memcpy(&shade_tris[in.first_tri + j].q[25], &mids[k], 4);      // the word write_shade_tri writes
    }
    return FRT_OK;
}
int SceneBuilder::set_light_emission(uint32_t light, const float color[3], float intensity) {
    if (!built) { error = "set_light_emission: scene is not built"; return FRT_ERR_STATE; }
    if (!color) { error = "set_light_emission: null colour"; return FRT_ERR_INVALID_ARG; }
    if (light >= lights.size()) { error = "set_light_emission: light " + std::to_string(light) + " out of range (" + std::to_string(lights.size()) + " lights)"; return FRT_ERR_INVALID_ARG; }
    const float em[4] = {color[0], color[1], color[2], intensity};
    memcpy(lights[light].emission, em, sizeof(em));
    const int i = light_instance(instances, light);
    if (i >= 0 && instances[(size_t)i].mat_id < materials.size()) light_emissive_factor(color, intensity, materials[instances[(size_t)i].mat_id].emissive_factor);
    return FRT_OK;
}
int SceneBuilder::set_texture(int kind, uint32_t layer, const uint8_t* rgba8) {
    if (!built) { error = "set_texture: scene is not built"; return FRT_ERR_STATE; }
    const std::string bad = check_set_texture(kind, layer, rgba8, color_textures.size(), data_textures.size());
    if (!bad.empty()) { error = "set_texture: " + bad; return FRT_ERR_INVALID_ARG; }
    (kind == 0 ? color_textures : data_textures)[layer].assign(rgba8, rgba8 + kTexBytes);
    return FRT_OK;
}

// ---------------------------------------------------------------------------------------------- adding and removing instances
int check_add_instances(uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* mats, const std::vector<uint32_t>& mesh_tris, size_t num_materials,
                        uint64_t num_tris, std::string& why) {
    if (n > 0 && (!mesh_ids || !mat_ids || !mats)) { why = "null mesh ids, material ids or matrices"; return FRT_ERR_INVALID_ARG; }
    uint64_t total = num_tris;
    for (uint32_t k = 0; k < n; ++k) {
        if (mesh_ids[k] >= mesh_tris.size()) { why = "mesh id " + std::to_string(mesh_ids[k]) + " out of range (" + std::to_string(mesh_tris.size()) + " meshes)"; return FRT_ERR_INVALID_ARG; }
        if (mat_ids[k] >= num_materials) { why = "material id " + std::to_string(mat_ids[k]) + " out of range (" + std::to_string(num_materials) + " materials)"; return FRT_ERR_INVALID_ARG; }
        float w2o[9]; uint32_t flip;
        if (!instance_inverse(mats + 16 * (size_t)k, w2o, flip)) { why = "matrix " + std::to_string(k) + " has a non-finite entry or a singular 3x3"; return FRT_ERR_INVALID_ARG; }
        total += mesh_tris[mesh_ids[k]];
    }
    if (total > kMaxSceneTris) { why = std::to_string(total) + " triangles would result, " + std::to_string(kMaxSceneTris) + " is the limit"; return FRT_ERR_LIMIT; }
    return FRT_OK;
}
int check_remove_instances(uint32_t n, const uint32_t* ids, const std::vector<InstanceRec>& instances, std::vector<uint32_t>& removed, std::string& why) {
    removed.clear();
    if (n > 0 && !ids) { why = "null ids"; return FRT_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < n; ++k) {
        if (ids[k] >= instances.size()) { why = "instance id " + std::to_string(ids[k]) + " out of range (" + std::to_string(instances.size()) + " instances)"; return FRT_ERR_INVALID_ARG; }
        if (instances[ids[k]].light >= 0) {
            why = "instance " + std::to_string(ids[k]) + " was registered with light " + std::to_string(instances[ids[k]].light) + ": its material and its light record carry links to it";
            return FRT_ERR_INVALID_ARG;
        }
    }
    removed.assign(ids, ids + n);
    std::sort(removed.begin(), removed.end());
    removed.erase(std::unique(removed.begin(), removed.end()), removed.end());
    if (n > 0 && removed.size() == instances.size()) { removed.clear(); why = "every instance would be removed (a scene without triangles cannot be built)"; return FRT_ERR_INVALID_ARG; }
    return FRT_OK;
}

int SceneBuilder::add_instances(uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* mats) {
    if (!built) { error = "add_instances: scene is not built"; return FRT_ERR_STATE; }
    std::vector<uint32_t> mesh_tris(mesh_index_counts.size());
    for (size_t m = 0; m < mesh_tris.size(); ++m) mesh_tris[m] = mesh_index_counts[m] / 3u;
    std::string why;
    if (const int rc = check_add_instances(n, mesh_ids, mat_ids, mats, mesh_tris, materials.size(), tris.size(), why)) { error = "add_instances: " + why; return rc; }
    const size_t first = instances.size();
    if (n == 0) return (int)first;
    for (uint32_t k = 0; k < n; ++k) {
        Mat4 t; memcpy(t.m, mats + 16 * (size_t)k, sizeof(t.m));
        add_instance(mesh_ids[k], mat_ids[k], t);
    }
    build();
    if (!built) {      // (a tree the builder refuses: back to the list as it was, built the same way it had been)
        const std::string why_not = error;
        instances.resize(first);
        build();
        error = "add_instances: " + why_not + " (nothing changed)";
        return FRT_ERR_LIMIT;
    }
    return (int)first;
}

int SceneBuilder::remove_instances(uint32_t n, const uint32_t* ids) {
    if (!built) { error = "remove_instances: scene is not built"; return FRT_ERR_STATE; }
    std::vector<uint32_t> gone;
    std::string why;
    if (const int rc = check_remove_instances(n, ids, instances, gone, why)) { error = "remove_instances: " + why; return rc; }
    if (gone.empty()) return FRT_OK;
    const std::vector<InstanceRec> before = instances;
    size_t g = 0, w = 0;
    for (size_t i = 0; i < before.size(); ++i) {      // the survivors in their order (each keeps its light link: lights are not renumbered)
        if (g < gone.size() && gone[g] == i) { ++g; continue; }
        instances[w++] = before[i];
    }
    instances.resize(w);
    build();
    if (!built) {
        const std::string why_not = error;
        instances = before;
        build();
        error = "remove_instances: " + why_not + " (nothing changed)";
        return FRT_ERR_LIMIT;
    }
    return FRT_OK;
}

// ---------------------------------------------------------------------------------------------- new meshes, materials, layers, lights
int check_add_meshes(uint32_t n, const frt_mesh_data* meshes, uint64_t num_verts, uint64_t num_indices, std::string& why) {
    if (n > 0 && !meshes) { why = "null meshes"; return FRT_ERR_INVALID_ARG; }
    uint64_t verts = num_verts, indices = num_indices;
    for (uint32_t k = 0; k < n; ++k) {
        const frt_mesh_data& m = meshes[k];
        const std::string which = "mesh " + std::to_string(k) + ": ";
        if (!m.pos4 || !m.attrs || !m.idx) { why = which + "null positions, attributes or indices"; return FRT_ERR_INVALID_ARG; }
        if (m.nverts == 0) { why = which + "no vertices"; return FRT_ERR_INVALID_ARG; }
        if (m.nidx == 0 || m.nidx % 3u != 0u) { why = which + std::to_string(m.nidx) + " indices (a positive multiple of 3 is needed)"; return FRT_ERR_INVALID_ARG; }
        for (uint32_t i = 0; i < m.nidx; ++i)
            if (m.idx[i] >= m.nverts) { why = which + "index " + std::to_string(i) + " is " + std::to_string(m.idx[i]) + ", the mesh has " + std::to_string(m.nverts) + " vertices"; return FRT_ERR_INVALID_ARG; }
        const std::string bad = check_mesh_vertices(m.pos4, m.attrs, m.nverts, m.nverts);
        if (!bad.empty()) { why = which + bad; return FRT_ERR_INVALID_ARG; }
        verts += m.nverts; indices += m.nidx;      // (n < 2^32 terms of less than 2^32 each: no overflow in 64 bits)
    }
    if (verts > kMaxPoolElems) { why = std::to_string(verts) + " vertices would result, " + std::to_string(kMaxPoolElems) + " is the limit"; return FRT_ERR_LIMIT; }
    if (indices > kMaxPoolElems) { why = std::to_string(indices) + " indices would result, " + std::to_string(kMaxPoolElems) + " is the limit"; return FRT_ERR_LIMIT; }
    return FRT_OK;
}
int check_add_materials(uint32_t n, const frt_material* mats, size_t num_materials, size_t color_layers, size_t data_layers, size_t num_lights, std::string& why) {
    if (n > 0 && !mats) { why = "null materials"; return FRT_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < n; ++k) {
        const std::string bad = check_material(mats[k], color_layers, data_layers, num_lights);
        if (!bad.empty()) { why = "material " + std::to_string(k) + ": " + bad; return FRT_ERR_INVALID_ARG; }
    }
    if ((uint64_t)num_materials + n > kMaxMaterials) { why = "more than 65535 materials (custom index packs 16 bits, builder.rs:184)"; return FRT_ERR_LIMIT; }
    return FRT_OK;
}
int check_add_texture(int kind, const uint8_t* rgba8, size_t color_layers, size_t data_layers, std::string& why) {
    if (kind != 0 && kind != 1) { why = "kind must be 0 (colour) or 1 (data)"; return FRT_ERR_INVALID_ARG; }
    if (!rgba8) { why = "null pixels"; return FRT_ERR_INVALID_ARG; }
    if ((kind == 0 ? color_layers : data_layers) >= kMaxTextureLayers) { why = "too many texture layers"; return FRT_ERR_LIMIT; }
    return FRT_OK;
}
int check_add_lights(uint32_t n, const frt_light* lights, std::string& why) {
    if (n > 0 && !lights) { why = "null lights"; return FRT_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < n; ++k) {
        const frt_light& l = lights[k];
        const float f[14] = {l.position[0], l.position[1], l.position[2], l.u[0], l.u[1], l.u[2], l.area, l.v[0], l.v[1], l.v[2], l.emission[0], l.emission[1], l.emission[2], l.emission[3]};
        for (float x : f) if (!std::isfinite(x)) { why = "light " + std::to_string(k) + " has a non-finite field"; return FRT_ERR_INVALID_ARG; }
        if (!(l.area > 0.0f)) { why = "light " + std::to_string(k) + " has no area"; return FRT_ERR_INVALID_ARG; }
    }
    return FRT_OK;
}
void pack_mesh_appends(uint32_t n, const frt_mesh_data* meshes, uint32_t num_verts, uint32_t num_indices, std::vector<MeshAppend>& rec, uint32_t& new_verts, uint32_t& new_indices) {
    rec.assign(n, MeshAppend{});
    new_verts = new_indices = 0;
    for (uint32_t k = 0; k < n; ++k) {
        rec[k] = MeshAppend{num_verts + new_verts, num_indices + new_indices, meshes[k].nverts, meshes[k].nidx, new_verts, new_indices, {0u, 0u}};
        new_verts += meshes[k].nverts; new_indices += meshes[k].nidx;
    }
}
uint32_t grown_capacity(uint64_t have, uint64_t need, uint64_t limit) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(need, 2ull * have), limit); }
uint32_t grown_layer_capacity(uint64_t have, uint64_t need) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(need, have + std::max<uint64_t>(4, have / 2)), kMaxTextureLayers); }

// ---------------------------------------------------------------------------------------------- removing materials, meshes, lights, layers
std::vector<uint32_t> removal_map(size_t count, const std::vector<uint32_t>& removed) {
    std::vector<uint32_t> map(count);
    size_t g = 0;
    for (size_t i = 0; i < count; ++i) {
        if (g < removed.size() && removed[g] == i) { map[i] = kGone; ++g; }
        else map[i] = (uint32_t)(i - g);
    }
    return map;
}
// The distinct ids of a call, ascending; false (with `why`) for a null pointer or an id out of range.
static bool distinct_ids(uint32_t n, const uint32_t* ids, size_t count, const char* what, std::vector<uint32_t>& out, std::string& why) {
    out.clear();
    if (n > 0 && !ids) { why = "null ids"; return false; }
    for (uint32_t k = 0; k < n; ++k)
        if (ids[k] >= count) { why = std::string(what) + " id " + std::to_string(ids[k]) + " out of range (" + std::to_string(count) + ")"; return false; }
    out.assign(ids, ids + n);
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return true;
}
int check_remove_materials(uint32_t n, const uint32_t* ids, size_t num_materials, const std::vector<InstanceRec>& instances, std::vector<uint32_t>& removed, std::string& why) {
    if (!distinct_ids(n, ids, num_materials, "material", removed, why)) return FRT_ERR_INVALID_ARG;
    for (size_t i = 0; i < instances.size(); ++i) {
        const InstanceRec& in = instances[i];
        if (!std::binary_search(removed.begin(), removed.end(), in.mat_id)) continue;
        if (in.light >= 0) why = "material " + std::to_string(in.mat_id) + " was made with light " + std::to_string(in.light) + " by register_*_light: remove the light instead";
        else why = "instance " + std::to_string(i) + " still uses material " + std::to_string(in.mat_id);
        removed.clear();
        return FRT_ERR_INVALID_ARG;
    }
    return FRT_OK;
}
int check_remove_meshes(uint32_t n, const uint32_t* ids, size_t num_meshes, const std::vector<InstanceRec>& instances, std::vector<uint32_t>& removed, std::string& why) {
    if (!distinct_ids(n, ids, num_meshes, "mesh", removed, why)) return FRT_ERR_INVALID_ARG;
    for (size_t i = 0; i < instances.size(); ++i)
        if (std::binary_search(removed.begin(), removed.end(), instances[i].mesh_id)) {
            why = "instance " + std::to_string(i) + " still uses mesh " + std::to_string(instances[i].mesh_id);
            removed.clear();
            return FRT_ERR_INVALID_ARG;
        }
    return FRT_OK;
}
int check_remove_lights(uint32_t n, const uint32_t* ids, size_t num_lights, const frt_material* materials, size_t num_materials, const std::vector<InstanceRec>& instances,
                        LightRemoval& out, std::string& why) {
    out = LightRemoval();
    if (!distinct_ids(n, ids, num_lights, "light", out.lights, why)) return FRT_ERR_INVALID_ARG;
    if (out.lights.empty()) return FRT_OK;
    if (!materials && num_materials > 0) { out = LightRemoval(); why = "null materials"; return FRT_ERR_INVALID_ARG; }
    auto refuse = [&](const std::string& w) { why = w; out = LightRemoval(); return (int)FRT_ERR_INVALID_ARG; };
    for (size_t i = 0; i < instances.size(); ++i) {      // the composites register_*_light made: the instance and its material leave with the light
        const InstanceRec& in = instances[i];
        if (in.light < 0 || !std::binary_search(out.lights.begin(), out.lights.end(), (uint32_t)in.light)) continue;
        out.instances.push_back((uint32_t)i);
        if (in.mat_id < num_materials) out.materials.push_back(in.mat_id);
    }
    std::sort(out.materials.begin(), out.materials.end());
    out.materials.erase(std::unique(out.materials.begin(), out.materials.end()), out.materials.end());
    if (!out.instances.empty() && out.instances.size() == instances.size()) return refuse("every instance would be removed (a scene without triangles cannot be built)");
    for (size_t i = 0; i < instances.size(); ++i) {
        if (std::binary_search(out.instances.begin(), out.instances.end(), (uint32_t)i)) continue;
        if (std::binary_search(out.materials.begin(), out.materials.end(), instances[i].mat_id))
            return refuse("instance " + std::to_string(i) + " still uses material " + std::to_string(instances[i].mat_id) + ", which a removed light was registered with");
    }
    for (size_t m = 0; m < num_materials; ++m) {
        if (std::binary_search(out.materials.begin(), out.materials.end(), (uint32_t)m)) continue;
        const int32_t li = materials[m].light_index;
        if (li >= 0 && std::binary_search(out.lights.begin(), out.lights.end(), (uint32_t)li))
            return refuse("light_index of material " + std::to_string(m) + " still names light " + std::to_string(li));
    }
    return FRT_OK;
}
int check_remove_texture(int kind, uint32_t layer, size_t color_layers, size_t data_layers, const frt_material* materials, size_t num_materials, std::string& why) {
    if (kind != 0 && kind != 1) { why = "kind must be 0 (colour) or 1 (data)"; return FRT_ERR_INVALID_ARG; }
    const size_t layers = kind == 0 ? color_layers : data_layers;
    const std::string name = std::string(kind == 0 ? "colour" : "data") + " layer " + std::to_string(layer);
    if (layer >= layers) { why = name + " does not exist (" + std::to_string(layers) + " layers)"; return FRT_ERR_INVALID_ARG; }
    if (layer < kBuilderLayers) { why = name + " is one of the layers every scene starts with"; return FRT_ERR_INVALID_ARG; }
    if (!materials && num_materials > 0) { why = "null materials"; return FRT_ERR_INVALID_ARG; }
    for (size_t m = 0; m < num_materials; ++m) {
        const frt_material& a = materials[m];
        const uint32_t color[2] = {a.tex_info_0 & 0xFFFFu, a.tex_info_1 >> 16}, data[3] = {a.tex_info_0 >> 16, a.tex_info_1 & 0xFFFFu, a.tex_info_2 & 0xFFFFu};
        bool used = false;
        if (kind == 0) for (uint32_t s : color) used |= s == layer;
        else for (uint32_t s : data) used |= s == layer;
        if (used) { why = "material " + std::to_string(m) + " still names " + name; return FRT_ERR_INVALID_ARG; }
    }
    return FRT_OK;
}
static uint32_t slot_without(uint32_t slot, uint32_t layer) { return slot != 0xFFFFu && layer != kGone && slot > layer ? slot - 1u : slot; }
void remap_material(frt_material& m, const std::vector<uint32_t>& light_map, uint32_t color_layer, uint32_t data_layer) {
    if (m.light_index >= 0 && (size_t)m.light_index < light_map.size() && light_map[(size_t)m.light_index] != kGone) m.light_index = (int32_t)light_map[(size_t)m.light_index];
    m.tex_info_0 = slot_without(m.tex_info_0 & 0xFFFFu, color_layer) | (slot_without(m.tex_info_0 >> 16, data_layer) << 16);
    m.tex_info_1 = slot_without(m.tex_info_1 & 0xFFFFu, data_layer) | (slot_without(m.tex_info_1 >> 16, color_layer) << 16);
    m.tex_info_2 = slot_without(m.tex_info_2 & 0xFFFFu, data_layer) | (m.tex_info_2 & 0xFFFF0000u);
}
void pack_mesh_removal(const std::vector<uint32_t>& removed, const std::vector<uint32_t>& vert_offset, const std::vector<uint32_t>& vert_count,
                       const std::vector<uint32_t>& index_offset, const std::vector<uint32_t>& index_count,
                       std::vector<RemovedSpan>& meshes, std::vector<RemovedSpan>& verts, std::vector<RemovedSpan>& indices) {
    meshes.clear(); verts.clear(); indices.clear();
    uint32_t vgone = 0, igone = 0;
    for (size_t k = 0; k < removed.size(); ++k) {
        const uint32_t m = removed[k];
        meshes.push_back(RemovedSpan{m - (uint32_t)k, (uint32_t)k + 1u});
        verts.push_back(RemovedSpan{vert_offset[m] - vgone, vgone + vert_count[m]});
        indices.push_back(RemovedSpan{index_offset[m] - igone, igone + index_count[m]});
        vgone += vert_count[m]; igone += index_count[m];
    }
}

// The four host forms share their end: build() over the edited lists; a tree the builder refuses puts the lists back as `undo` holds them.
namespace {
struct Lists {
    std::vector<frt_material> materials; std::vector<frt_vertex_attr> attributes; std::vector<uint32_t> indices; std::vector<MeshInfo> mesh_infos; std::vector<frt_light> lights;
    std::vector<std::vector<float>> mesh_positions; std::vector<uint32_t> mesh_index_counts; std::vector<InstanceRec> instances;
};
Lists lists_of(const SceneBuilder& b) { return Lists{b.materials, b.attributes, b.indices, b.mesh_infos, b.lights, b.mesh_positions, b.mesh_index_counts, b.instances}; }
int rebuild_or_undo(SceneBuilder& b, Lists& undo, const char* what) {
    b.build();
    if (b.built) return FRT_OK;
    const std::string why_not = b.error;
    b.materials.swap(undo.materials); b.attributes.swap(undo.attributes); b.indices.swap(undo.indices); b.mesh_infos.swap(undo.mesh_infos); b.lights.swap(undo.lights);
    b.mesh_positions.swap(undo.mesh_positions); b.mesh_index_counts.swap(undo.mesh_index_counts); b.instances.swap(undo.instances);
    b.build();
    b.error = std::string(what) + ": " + why_not + " (nothing changed)";
    return FRT_ERR_LIMIT;
}
}

int SceneBuilder::remove_materials(uint32_t n, const uint32_t* ids) {
    if (!built) { error = "remove_materials: scene is not built"; return FRT_ERR_STATE; }
    std::vector<uint32_t> gone;
    std::string why;
    if (const int rc = check_remove_materials(n, ids, materials.size(), instances, gone, why)) { error = "remove_materials: " + why; return rc; }
    if (gone.empty()) return FRT_OK;
    Lists undo = lists_of(*this);
    const std::vector<uint32_t> map = removal_map(materials.size(), gone);
    remove_elements(materials, gone);
    for (InstanceRec& in : instances) if (in.mat_id < map.size()) in.mat_id = map[in.mat_id];
    return rebuild_or_undo(*this, undo, "remove_materials");
}
// A per-mesh list of bindings (empty, or as long as the last bound mesh asks) loses the entries of the meshes `gone`: the survivors' follow their new ids.
template <class T>
static void bindings_follow_mesh_ids(std::vector<T>& list, size_t old_meshes, const std::vector<uint32_t>& gone) {
    if (list.empty()) return;
    list.resize(old_meshes);
    remove_elements(list, gone);
}
int SceneBuilder::remove_meshes(uint32_t n, const uint32_t* ids) {
    if (!built) { error = "remove_meshes: scene is not built"; return FRT_ERR_STATE; }
    std::vector<uint32_t> gone;
    std::string why;
    if (const int rc = check_remove_meshes(n, ids, mesh_infos.size(), instances, gone, why)) { error = "remove_meshes: " + why; return rc; }
    if (gone.empty()) return FRT_OK;
    Lists undo = lists_of(*this);
    const std::vector<uint32_t> map = removal_map(mesh_infos.size(), gone);
    std::vector<frt_vertex_attr> attrs; std::vector<uint32_t> idx; std::vector<MeshInfo> infos;
    for (size_t m = 0; m < mesh_infos.size(); ++m) {      // the pools as add_mesh lays the surviving meshes out
        if (map[m] == kGone) continue;
        const size_t nv = mesh_positions[m].size() / 4, ni = mesh_index_counts[m];
        infos.push_back(MeshInfo{(uint32_t)attrs.size(), (uint32_t)idx.size(), {0, 0}});
        attrs.insert(attrs.end(), attributes.begin() + mesh_infos[m].vertex_offset, attributes.begin() + mesh_infos[m].vertex_offset + nv);
        idx.insert(idx.end(), indices.begin() + mesh_infos[m].index_offset, indices.begin() + mesh_infos[m].index_offset + ni);
    }
    attributes.swap(attrs); indices.swap(idx); mesh_infos.swap(infos);
    remove_elements(mesh_positions, gone); remove_elements(mesh_index_counts, gone);
    for (InstanceRec& in : instances) in.mesh_id = map[in.mesh_id];
    const int rc = rebuild_or_undo(*this, undo, "remove_meshes");
    if (rc == FRT_OK) {      // the skins and the morph targets follow the mesh ids (a call that was undone leaves them)
        bindings_follow_mesh_ids(mesh_skins, map.size(), gone);
        bindings_follow_mesh_ids(mesh_morphs, map.size(), gone);
    }
    return rc;
}
int SceneBuilder::remove_lights(uint32_t n, const uint32_t* ids) {
    if (!built) { error = "remove_lights: scene is not built"; return FRT_ERR_STATE; }
    LightRemoval rem;
    std::string why;
    if (const int rc = check_remove_lights(n, ids, lights.size(), materials.data(), materials.size(), instances, rem, why)) { error = "remove_lights: " + why; return rc; }
    if (rem.lights.empty()) return FRT_OK;
    Lists undo = lists_of(*this);
    const std::vector<uint32_t> light_map = removal_map(lights.size(), rem.lights), mat_map = removal_map(materials.size(), rem.materials);
    remove_elements(instances, rem.instances); remove_elements(materials, rem.materials); remove_elements(lights, rem.lights);
    for (InstanceRec& in : instances) {
        if (in.mat_id < mat_map.size()) in.mat_id = mat_map[in.mat_id];
        if (in.light >= 0 && (size_t)in.light < light_map.size()) in.light = (int32_t)light_map[(size_t)in.light];
    }
    for (frt_material& m : materials) remap_material(m, light_map, kGone, kGone);
    return rebuild_or_undo(*this, undo, "remove_lights");
}
int SceneBuilder::remove_texture(int kind, uint32_t layer) {
    if (!built) { error = "remove_texture: scene is not built"; return FRT_ERR_STATE; }
    std::string why;
    if (const int rc = check_remove_texture(kind, layer, color_textures.size(), data_textures.size(), materials.data(), materials.size(), why)) { error = "remove_texture: " + why; return rc; }
    auto& layers = kind == 0 ? color_textures : data_textures;
    layers.erase(layers.begin() + layer);
    for (frt_material& m : materials) remap_material(m, {}, kind == 0 ? layer : kGone, kind == 1 ? layer : kGone);      // (nothing build() derives names a layer)
    return FRT_OK;
}

void SceneBuilder::build() {
    error.clear();
    // Texture layers and light indices reach the kernels unchecked (sample_layer: base + layer * 4 MiB): validate them here, once.
    // wgpu would reject an out-of-range layer at bind time / clamp the fetch; here it would be an out-of-bounds read on the GPU.
    for (size_t i = 0; i < materials.size() && error.empty(); ++i) {
        const std::string bad = check_material(materials[i], color_textures.size(), data_textures.size(), lights.size());
        if (!bad.empty()) error = "material " + std::to_string(i) + ": " + bad;
    }
    if (!error.empty()) { built = false; return; }
    flatten();
    build_bvh2();
    build_gpu_layout();
    built = error.empty();
}

// ---------------------------------------------------------------------------------------------- scenes.rs
namespace scenes {
static const float kPi = 3.14159265358979323846f, kHalfPi = 1.57079632679489661923f;

void create_cornell_box(SceneBuilder& b) {
    uint32_t plane = b.add_mesh(geometry::create_plane());
    uint32_t cube = b.add_mesh(geometry::create_cube());
    uint32_t sphere = b.add_mesh(geometry::create_sphere(3));
    uint32_t crystal = b.add_mesh(geometry::create_crystal());

    uint32_t red = b.add_material(MaterialBuilder(0.65f, 0.05f, 0.05f, 1.0f));
    uint32_t green = b.add_material(MaterialBuilder(0.12f, 0.45f, 0.15f, 1.0f));
    uint32_t white = b.add_material(MaterialBuilder(0.73f, 0.73f, 0.73f, 1.0f));
    uint32_t checker = b.add_material(MaterialBuilder(0.73f, 0.73f, 0.73f, 1.0f).roughness(0.99f).texture(1));
    uint32_t metal = b.add_material(MaterialBuilder(0.8f, 0.8f, 0.8f, 1.0f).metallic(0.01f));
    uint32_t glass = b.add_material(MaterialBuilder(0.5f, 0.8f, 1.0f, 1.0f).glass(1.5f));

    auto TRS = [](const Mat4& t, const Mat4& r, float s) { return mat4_mul(mat4_mul(t, r), mat4_scale(s, s, s)); };
    b.add_instance(plane, checker, mat4_mul(mat4_translation(0, -1, 0), mat4_scale(2, 2, 2)));                 // floor
    b.add_instance(plane, white, TRS(mat4_translation(0, 1, 0), mat4_rotation_x(kPi), 2.0f));                    // ceiling
    b.add_instance(plane, white, TRS(mat4_translation(0, 0, -1), mat4_rotation_x(kHalfPi), 2.0f));               // back
    b.add_instance(plane, red, TRS(mat4_translation(-1, 0, 0), mat4_rotation_z(-kHalfPi), 2.0f));                // left
    b.add_instance(plane, green, TRS(mat4_translation(1, 0, 0), mat4_rotation_z(kHalfPi), 2.0f));                // right
    const float white_light[3] = {1.0f, 1.0f, 1.0f};
    b.register_quad_light(plane, TRS(mat4_translation(0, 0.99f, 0), mat4_rotation_x(kPi), 0.5f), white_light, 10.0f);
    b.add_instance(crystal, glass, mat4_mul(mat4_translation(0.4f, -0.5f, 0.3f), mat4_scale(0.5f, 0.5f, 0.5f)));
    const float blue_light[3] = {0.02f, 0.02f, 0.9f};
    b.register_sphere_light(sphere, mat4_mul(mat4_translation(0.4f, -0.5f, 0.3f), mat4_scale(0.1f, 0.1f, 0.1f)), blue_light, 10.0f);
    b.add_instance(cube, metal, mat4_mul(mat4_mul(mat4_translation(-0.35f, -0.4f + 0.002f, -0.3f), mat4_rotation_y(0.4f)), mat4_scale(0.6f, 1.2f, 0.6f)));
    b.build();
}

static void hsv_to_rgb(float h, float s, float v, float rgb[3]) {   // scenes.rs:226-246
    float c = v * s, x = c * (1.0f - fabsf(fmodf(h * 6.0f, 2.0f) - 1.0f)), m = v - c;
    int sector = h < 1.0f / 6.0f ? 0 : h < 2.0f / 6.0f ? 1 : h < 3.0f / 6.0f ? 2 : h < 4.0f / 6.0f ? 3 : h < 5.0f / 6.0f ? 4 : 5;
    const float table[6][3] = {{c, x, 0}, {x, c, 0}, {0, c, x}, {0, x, c}, {x, 0, c}, {c, 0, x}};
    for (int i = 0; i < 3; ++i) rgb[i] = table[sector][i] + m;
}

void create_restir_scene(SceneBuilder& b) {
    uint32_t plane = b.add_mesh(geometry::create_plane());
    uint32_t sphere = b.add_mesh(geometry::create_sphere(2));
    uint32_t cube = b.add_mesh(geometry::create_cube());
    uint32_t mat_floor = b.add_material(MaterialBuilder(0.73f, 0.73f, 0.73f, 1.0f).roughness(0.99f));
    uint32_t mat_wall = b.add_material(MaterialBuilder(0.73f, 0.73f, 0.73f, 1.0f).roughness(0.99f));
    uint32_t mat_metal = b.add_material(MaterialBuilder(1, 1, 1, 1).metallic(0.2f));
    b.add_instance(plane, mat_floor, mat4_mul(mat4_translation(0, -1, 0), mat4_scale(10, 10, 10)));
    b.add_instance(plane, mat_wall, mat4_mul(mat4_mul(mat4_translation(0, 5, -5), mat4_rotation_x(kHalfPi)), mat4_scale(10, 10, 10)));
    const int rows = 10, cols = 10;
    const float spacing = 1.0f, radius = 0.05f, strength = 20.0f;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            float x = ((float)c - (float)cols / 2.0f) * spacing, z = ((float)r - (float)rows / 2.0f) * spacing, y = -0.9f;
            float col[3];
            hsv_to_rgb((float)(r * cols + c) / (float)(rows * cols), 0.8f, 1.0f, col);
            uint32_t mat = b.add_material(MaterialBuilder(col[0], col[1], col[2], 1.0f).light_index(r * cols + c)
                                              .emissive_factor(col[0] * strength, col[1] * strength, col[2] * strength));
            b.add_instance(sphere, mat, mat4_mul(mat4_translation(x, y, z), mat4_scale(radius, radius, radius)));
            const float pos[3] = {x, y, z}, em[4] = {col[0], col[1], col[2], strength};
            b.add_sphere_light(pos, radius, em);
        }
    b.add_instance(cube, mat_metal, mat4_mul(mat4_translation(0, -0.5f, 0), mat4_scale(0.5f, 0.5f, 0.5f)));
    b.build();
}
} // namespace scenes

// ---------------------------------------------------------------------------------------------- camera.rs
// CameraController::build_uniform (camera.rs:207-256) for any pose, jitter and previous view-projection.
// prev_view_proj == null stands for the controller's initial Mat4::IDENTITY ("first frame": the unjittered view_proj is sent, :233-238).
// unjittered_out (may be null) receives the second tuple element, which State stores as the next frame's prev_view_proj (state.rs:172).
void camera_build_uniform(const float position[3], float yaw, float pitch, const float* prev_view_proj, float aspect, uint32_t frame_count,
                          uint32_t num_lights, float jitter_x, float jitter_y, frt_camera_uniform* out, float* unjittered_out) {
    const float eye[3] = {position[0], position[1], position[2]};
    const float rad_per_deg = 3.14159265358979323846f / 180.0f;
    float fwd[3] = {cosf(pitch) * cosf(yaw), sinf(pitch), cosf(pitch) * sinf(yaw)};
    v3_normalize_glam(fwd);
    // Mat4::look_at_rh(eye, eye + fwd, Y) -> look_to_rh(eye, (eye + fwd) - eye, Y)
    float f[3] = {(eye[0] + fwd[0]) - eye[0], (eye[1] + fwd[1]) - eye[1], (eye[2] + fwd[2]) - eye[2]};
    v3_normalize_glam(f);
    float s[3] = {f[1] * 0.0f - f[2] * 1.0f, f[2] * 0.0f - f[0] * 0.0f, f[0] * 1.0f - f[1] * 0.0f};   // f x (0,1,0)
    v3_normalize_glam(s);
    float u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};   // s x f
    auto dot3 = [](const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    Mat4 view = mat4_identity();
    for (int c = 0; c < 3; ++c) { view.m[4 * c] = s[c]; view.m[4 * c + 1] = u[c]; view.m[4 * c + 2] = -f[c]; }
    view.m[12] = -dot3(eye, s); view.m[13] = -dot3(eye, u); view.m[14] = dot3(eye, f);
    // Mat4::perspective_rh(45 deg, aspect, 0.1, 100): depth 0..1
    float half = 0.5f * (45.0f * rad_per_deg);
    float hh = cosf(half) / sinf(half), ww = hh / aspect, rr = 100.0f / (0.1f - 100.0f);
    Mat4 proj_base{};
    proj_base.m[0] = ww; proj_base.m[5] = hh; proj_base.m[10] = rr; proj_base.m[11] = -1.0f; proj_base.m[14] = rr * 0.1f;
    Mat4 vp_unjittered = mat4_mul(proj_base, view);
    Mat4 proj = proj_base;
    proj.m[8] += jitter_x;      // proj_cols[2][0] += jitter.0 (:226): shear of the projection
    proj.m[9] += jitter_y;      // proj_cols[2][1] += jitter.1 (:227)
    Mat4 vp = mat4_mul(proj, view), vi = mat4_inverse(view), pi = mat4_inverse(proj);
    memset(out, 0, sizeof(*out));
    memcpy(out->view_proj, vp.m, 64); memcpy(out->view_inverse, vi.m, 64); memcpy(out->proj_inverse, pi.m, 64);
    memcpy(out->prev_view_proj, prev_view_proj ? prev_view_proj : vp_unjittered.m, 64);
    out->view_pos[0] = eye[0]; out->view_pos[1] = eye[1]; out->view_pos[2] = eye[2]; out->view_pos[3] = 1.0f;
    out->frame_count = frame_count; out->num_lights = num_lights;
    if (unjittered_out) memcpy(unjittered_out, vp_unjittered.m, 64);
}
// CameraController::get_halton_jitter (camera.rs:182-205). The reference multiplies the Halton offsets by 0 (:202-203) — `scale`
// stands for that literal: 0 reproduces the shipped reference, 1 is the sequence the comment above it describes.
void camera_halton_jitter(uint32_t index, uint32_t width, uint32_t height, float scale, float out[2]) {
    auto halton = [](uint32_t i, uint32_t base) {
        float f = 1.0f, r = 0.0f;
        while (i > 0) { f /= (float)base; r += f * (float)(i % base); i /= base; }
        return r;
    };
    float hx = halton(index + 1u, 2u) - 0.5f, hy = halton(index + 1u, 3u) - 0.5f;
    out[0] = (hx * scale) / (float)width;
    out[1] = (hy * scale) / (float)height;
}
void camera_default(float aspect, uint32_t frame_count, uint32_t num_lights, frt_camera_uniform* out) {
    // CameraController::new (camera.rs:40-42) + build_uniform (:207-256), jitter = 0 (:202-203), prev_view_proj = IDENTITY
    // on the first call -> the unjittered view_proj; with a static camera it stays that value (state.rs:172).
    const float eye[3] = {0.0f, 0.0f, 3.0f};
    const float rad_per_deg = 3.14159265358979323846f / 180.0f;
    camera_build_uniform(eye, -90.0f * rad_per_deg, 0.0f, nullptr, aspect, frame_count, num_lights, 0.0f, 0.0f, out, nullptr);
}

} // namespace frt
