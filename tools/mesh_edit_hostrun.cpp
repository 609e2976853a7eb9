// mesh_edit_hostrun.cpp — the host half of adding meshes, materials, texture layers and lights to a renderer's replica as a stand-alone
// program to run under a sanitiser: the validation functions of frt_scene.cpp and the layout arithmetic of a call (destination bases, prefix sums, the
// 32-byte records, the capacities), over the cases the GPU tests run. It links the host scene sources only (no device code, nothing loaded into an
// interpreter).
//   hipcc --cuda-host-only -x hip -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Iinclude \
//       tools/mesh_edit_hostrun.cpp fast-raytracing-wgpu_amd/csrc/frt_scene.cpp fast-raytracing-wgpu_amd/csrc/frt_bvh.cpp \
//       -fsanitize=address,undefined -o mesh_edit_hostrun && ./mesh_edit_hostrun
// (host only: frt_math.hpp wants the HIP headers, hence hipcc.) Exit status 0 and "ok" when every step behaved. Run it on a CPU machine.
#include "../fast-raytracing-wgpu_amd/csrc/frt_scene.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace frt;

static void expect(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "FAILED: %s\n", what); exit(1); }
}
static frt_mesh_data data_of(const Geometry& g) {
    return frt_mesh_data{g.positions.data(), g.attributes.data(), g.indices.data(), (uint32_t)g.attributes.size(), (uint32_t)g.indices.size()};
}
static Geometry pyramid() {      // 5 vertices, 4 triangles: odd counts, so the mesh behind it starts at an unaligned base
    Geometry g;
    const float P[5][3] = {{-0.5f, 0, -0.5f}, {0.5f, 0, -0.5f}, {0.5f, 0, 0.5f}, {-0.5f, 0, 0.5f}, {0, 0.6f, 0}};
    for (auto& p : P) {
        g.positions.insert(g.positions.end(), {p[0], p[1], p[2], 1.0f});
        frt_vertex_attr a{};
        const float n[3] = {p[0], 0.5f, p[2]};
        geometry::encode_octahedral_normal(n, a.normal);
        a.tangent[0] = a.tangent[3] = 1.0f;
        g.attributes.push_back(a);
    }
    g.indices = {0, 4, 1, 1, 4, 2, 2, 4, 3, 3, 4, 0};
    return g;
}
static Geometry triangle() {
    Geometry g = geometry::create_plane();
    g.positions.resize(12); g.attributes.resize(3); g.indices = {0, 1, 2};
    return g;
}

// The records of a call against what SceneBuilder::add_mesh makes of the same meshes.
static void check_layout(SceneBuilder& b, const std::vector<Geometry>& meshes) {
    std::vector<frt_mesh_data> d;
    for (const Geometry& g : meshes) d.push_back(data_of(g));
    const uint32_t verts = (uint32_t)b.attributes.size(), indices = (uint32_t)b.indices.size();
    std::string why;
    expect(check_add_meshes((uint32_t)d.size(), d.data(), verts, indices, why) == FRT_OK, "good meshes pass");
    std::vector<MeshAppend> rec;
    uint32_t nv = 0, ni = 0;
    pack_mesh_appends((uint32_t)d.size(), d.data(), verts, indices, rec, nv, ni);
    expect(rec.size() == meshes.size(), "one record per mesh");
    uint32_t vb = 0, ib = 0;
    for (size_t k = 0; k < meshes.size(); ++k) {
        const uint32_t id = b.add_mesh(meshes[k]);
        const MeshInfo& mi = b.mesh_infos[id];
        expect(rec[k].vert_base == mi.vertex_offset && rec[k].index_base == mi.index_offset, "the bases are the builder's offsets");
        expect(rec[k].nverts == meshes[k].attributes.size() && rec[k].nidx == meshes[k].indices.size() && rec[k].nidx == b.mesh_index_counts[id], "the counts");
        expect(rec[k].vert_begin == vb && rec[k].index_begin == ib && rec[k].pad[0] == 0 && rec[k].pad[1] == 0, "the prefix sums");
        vb += rec[k].nverts; ib += rec[k].nidx;
    }
    expect(nv == vb && ni == ib && verts + nv == b.attributes.size() && indices + ni == b.indices.size(), "the totals");
    // staging as frt_renderer_add_meshes lays it out: [records | positions | attributes | indices]; copy through it and compare with the builder's arrays
    const size_t pos_at = rec.size() * sizeof(MeshAppend), attr_at = pos_at + (size_t)nv * 16, idx_at = attr_at + (size_t)nv * sizeof(frt_vertex_attr);
    std::vector<uint8_t> block(idx_at + (size_t)ni * 4);
    expect(pos_at % 16 == 0 && attr_at % 16 == 0 && idx_at % 16 == 0, "every part of the block is 16-byte aligned");
    for (size_t k = 0; k < meshes.size(); ++k) {
        memcpy(block.data() + pos_at + (size_t)rec[k].vert_begin * 16, d[k].pos4, (size_t)d[k].nverts * 16);
        memcpy(block.data() + attr_at + (size_t)rec[k].vert_begin * sizeof(frt_vertex_attr), d[k].attrs, (size_t)d[k].nverts * sizeof(frt_vertex_attr));
        memcpy(block.data() + idx_at + (size_t)rec[k].index_begin * 4, d[k].idx, (size_t)d[k].nidx * 4);
    }
    expect(memcmp(block.data() + attr_at, b.attributes.data() + verts, (size_t)nv * sizeof(frt_vertex_attr)) == 0, "the staged attributes are the builder's");
    expect(memcmp(block.data() + idx_at, b.indices.data() + indices, (size_t)ni * 4) == 0, "the staged indices are the builder's");
}

int main() {
    SceneBuilder b;
    scenes::create_cornell_box(b);
    expect(b.built, "the Cornell Box builds");
    // case 1: three meshes in one call; case 2: nine calls of one mesh each, capacities doubling on the way
    check_layout(b, {triangle(), geometry::create_sphere(1), pyramid()});
    uint32_t cap = (uint32_t)b.mesh_infos.size(), growths = 0;
    for (int k = 0; k < 9; ++k) {
        check_layout(b, {k % 2 ? triangle() : pyramid()});
        if (b.mesh_infos.size() > cap) { const uint32_t had = cap; cap = grown_capacity(cap, b.mesh_infos.size(), kMaxPoolElems); expect(cap >= 2 * had && cap >= b.mesh_infos.size(), "a capacity at least doubles"); ++growths; }
    }
    expect(growths <= 4, "nine meshes grow the mesh pool at most four times");
    expect(grown_capacity(0xC0000000ull, 0xC0000001ull, kMaxPoolElems) == 0xFFFFFFFFu, "a capacity stops at the limit");
    expect(grown_layer_capacity(3, 4) == 7 && grown_layer_capacity(20, 21) == 30 && grown_layer_capacity(3, 9) == 9 && grown_layer_capacity(0xFFFD, 0xFFFE) == 0xFFFE, "texture arrays grow by max(4, count / 2) layers");
    b.build();
    expect(b.built, "the scene with the new meshes builds");

    // case 7: every refusal
    std::string why;
    const Geometry good = triangle();
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto refused = [&](frt_mesh_data m, int code, const char* what) {
        const frt_mesh_data two[2] = {data_of(good), m};      // (a good mesh in front: the check looks at every mesh)
        expect(check_add_meshes(1, &m, 100, 300, why) == code && !why.empty(), what);
        expect(check_add_meshes(2, two, 100, 300, why) == code, what);
    };
    frt_mesh_data m = data_of(good);
    expect(check_add_meshes(1, nullptr, 0, 0, why) == FRT_ERR_INVALID_ARG && check_add_meshes(0, nullptr, 0, 0, why) == FRT_OK, "null meshes; n == 0");
    m = data_of(good); m.pos4 = nullptr; refused(m, FRT_ERR_INVALID_ARG, "null positions");
    m = data_of(good); m.attrs = nullptr; refused(m, FRT_ERR_INVALID_ARG, "null attributes");
    m = data_of(good); m.idx = nullptr; refused(m, FRT_ERR_INVALID_ARG, "null indices");
    m = data_of(good); m.nverts = 0; refused(m, FRT_ERR_INVALID_ARG, "no vertices");
    m = data_of(good); m.nidx = 0; refused(m, FRT_ERR_INVALID_ARG, "no indices");
    const uint32_t four[4] = {0, 1, 2, 0}, beyond[3] = {0, 1, 3};
    m = data_of(good); m.idx = four; m.nidx = 4; refused(m, FRT_ERR_INVALID_ARG, "indices not a multiple of 3");
    m = data_of(good); m.idx = beyond; refused(m, FRT_ERR_INVALID_ARG, "an index out of range");
    Geometry bad = good; bad.positions[6] = nan;
    refused(data_of(bad), FRT_ERR_INVALID_ARG, "a non-finite position");
    bad = good; bad.attributes[2].tangent[1] = inf;
    refused(data_of(bad), FRT_ERR_INVALID_ARG, "a non-finite attribute");
    m = data_of(good);
    expect(check_add_meshes(1, &m, 0xFFFFFFFDull, 0, why) == FRT_ERR_LIMIT && check_add_meshes(1, &m, 0xFFFFFFFCull, 0xFFFFFFFCull, why) == FRT_OK, "vertex totals beyond 32 bits, summed in 64");
    expect(check_add_meshes(1, &m, 0, 0xFFFFFFFDull, why) == FRT_ERR_LIMIT, "index totals beyond 32 bits");

    frt_material fine = MaterialBuilder(1, 1, 1, 1), no_layer = MaterialBuilder(1, 1, 1, 1).texture(3), no_light = MaterialBuilder(1, 1, 1, 1).light_index(2);
    const frt_material pair[2] = {fine, no_layer};
    expect(check_add_materials(1, &fine, 8, 3, 3, 2, why) == FRT_OK && check_add_materials(0, nullptr, 8, 3, 3, 2, why) == FRT_OK, "a good material; n == 0");
    expect(check_add_materials(1, nullptr, 8, 3, 3, 2, why) == FRT_ERR_INVALID_ARG, "null materials");
    expect(check_add_materials(1, &no_layer, 8, 3, 3, 2, why) == FRT_ERR_INVALID_ARG && check_add_materials(1, &no_layer, 8, 4, 3, 2, why) == FRT_OK, "a layer that does not exist yet; after it was added");
    expect(check_add_materials(1, &no_light, 8, 3, 3, 2, why) == FRT_ERR_INVALID_ARG && check_add_materials(1, &no_light, 8, 3, 3, 3, why) == FRT_OK, "a light that does not exist yet; after it was added");
    expect(check_add_materials(2, pair, 8, 3, 3, 2, why) == FRT_ERR_INVALID_ARG, "the second of two materials");
    expect(check_add_materials(1, &fine, 0xFFFF, 3, 3, 2, why) == FRT_ERR_LIMIT && check_add_materials(1, &fine, 0xFFFE, 3, 3, 2, why) == FRT_OK, "the 65,536th material");

    const uint8_t px[4] = {0, 0, 0, 0};
    expect(check_add_texture(0, px, 3, 3, why) == FRT_OK && check_add_texture(1, px, 3, 3, why) == FRT_OK, "good layers");
    expect(check_add_texture(2, px, 3, 3, why) == FRT_ERR_INVALID_ARG && check_add_texture(-1, px, 3, 3, why) == FRT_ERR_INVALID_ARG && check_add_texture(0, nullptr, 3, 3, why) == FRT_ERR_INVALID_ARG, "kind; null pixels");
    expect(check_add_texture(0, px, 0xFFFE, 3, why) == FRT_ERR_LIMIT && check_add_texture(1, px, 0xFFFE, 3, why) == FRT_OK && check_add_texture(1, px, 3, 0xFFFE, why) == FRT_ERR_LIMIT &&
           check_add_texture(0, px, 0xFFFD, 3, why) == FRT_OK, "a 65,535th layer is refused, in either array");

    const float em[4] = {1.0f, 0.5f, 0.2f, 6.0f};
    const frt_light quad = quad_light_record(mat4_scale(0.4f, 0.4f, 0.4f), em), sphere = sphere_light_record(mat4_translation(0.1f, 0.2f, 0.3f), em);
    const frt_light both[2] = {quad, sphere};
    expect(check_add_lights(2, both, why) == FRT_OK && check_add_lights(0, nullptr, why) == FRT_OK && check_add_lights(1, nullptr, why) == FRT_ERR_INVALID_ARG, "good lights; n == 0; null");
    frt_light l = quad; l.u[1] = nan;
    expect(check_add_lights(1, &l, why) == FRT_ERR_INVALID_ARG, "a non-finite field");
    l = sphere; l.emission[3] = inf;
    expect(check_add_lights(1, &l, why) == FRT_ERR_INVALID_ARG, "a non-finite emission");
    l = sphere; l.area = 0.0f;
    const frt_light second[2] = {quad, l};
    expect(check_add_lights(1, &l, why) == FRT_ERR_INVALID_ARG && check_add_lights(2, second, why) == FRT_ERR_INVALID_ARG, "no area");
    l = quad; l.area = -1.0f;
    expect(check_add_lights(1, &l, why) == FRT_ERR_INVALID_ARG, "a negative area");
    // the material and the record register_*_light makes: the builder's own
    const float color[3] = {1.0f, 0.8f, 0.6f};
    SceneBuilder c;
    scenes::create_cornell_box(c);
    const size_t nl = c.lights.size();
    const frt_material lm = light_emissive_material(nl, color, 7.0f);
    c.register_quad_light(0, mat4_scale(0.3f, 0.3f, 0.3f), color, 7.0f);
    expect(memcmp(&lm, &c.materials.back(), sizeof(lm)) == 0 && c.materials.back().light_index == (int32_t)nl, "the emissive material is the builder's");
    puts("ok");
    return 0;
}
