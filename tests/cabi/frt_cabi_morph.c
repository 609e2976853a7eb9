/* Morph targets from plain C (include/frt.h: frt_scene_set_mesh_morph_targets, frt_scene_set_mesh_morph_weights, frt_scene_set_mesh_pose_ex and their
 * renderer forms): a one-quad scene is built, two targets are bound to its four vertices, and a morph leaves the world-space triangles where the contract
 * puts them; morph and skin compose. With the argument "gpu" the same binding and morphs go to a renderer on device 0, whose triangle slots are read back
 * and compared with the scene's, byte for byte. Without it: host calls only, runs without a device.
 *   gcc -std=c99 -I include tests/cabi/frt_cabi_morph.c -L fast-raytracing-wgpu_amd/lib -lfrt */
#include "frt.h"
#include <stdio.h>
#include <string.h>

#define CHECK(call) do { int rc_ = (call); if (rc_ < 0) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, frt_last_error()); return 1; } } while (0)
#define REFUSED(call, what) do { if ((call) != FRT_ERR_INVALID_ARG) { fprintf(stderr, "%s\n", what); return 1; } } while (0)

int main(int argc, char** argv) {
    const int gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
    const float pos[16] = {-1, 0, -1, 1,   1, 0, -1, 1,   1, 0, 1, 1,   -1, 0, 1, 1};
    const uint32_t idx[6] = {0, 2, 1, 0, 3, 2};
    const float white[4] = {1, 1, 1, 1};
    const float identity[16] = {1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1};
    /* target 0 lifts vertex 2 by one and vertex 3 by one half; target 1 lowers vertex 3 by one; vertices 0 and 1 never move */
    const float deltas[2 * 4 * 3] = {0, 0, 0,  0, 0, 0,  0, 1, 0,  0, 0.5f, 0,      0, 0, 0,  0, 0, 0,  0, 0, 0,  0, -1, 0};
    const float weights[2] = {0.5f, -0.25f};          /* vertex 2: 0 + 0.5 * 1 = 0.5; vertex 3: (0 + 0.5 * 0.5) + -0.25 * -1 = 0.5 */
    const float above[2] = {1.5f, 0.0f};              /* weights above 1 are used as given: vertex 2 at 1.5, vertex 3 at 0.75 */
    const uint16_t joints[16] = {0, 0, 0, 0,   0, 0, 0, 0,   1, 1, 1, 1,   1, 1, 1, 1};
    const float skin_w[16] = {1, 0, 0, 0,   1, 0, 0, 0,   1, 0, 0, 0,   1, 0, 0, 0};
    frt_vertex_attr attrs[4];
    frt_material mat;
    uint32_t counts[8];
    float tris[2 * 9], mats[32], bad[2];
    volatile float huge = 1.0e38f;
    frt_scene* s = frt_scene_create();
    if (!s) { fprintf(stderr, "scene: %s\n", frt_last_error()); return 1; }
    memset(attrs, 0, sizeof(attrs));
    bad[0] = 0.5f; bad[1] = huge * huge;                  /* an infinity */
    frt_material_default(white, &mat);
    CHECK(frt_scene_add_mesh(s, pos, 4, attrs, idx, 6));
    CHECK(frt_scene_add_material(s, &mat));
    if (frt_scene_set_mesh_morph_targets(s, 0, deltas, 4, 2) != FRT_ERR_STATE) { fprintf(stderr, "an unbuilt scene took targets\n"); return 1; }
    CHECK(frt_scene_add_instance(s, 0, 0, identity));
    CHECK(frt_scene_build(s));
    CHECK(frt_scene_counts(s, counts));
    if (counts[0] != 2) { fprintf(stderr, "%u triangles\n", counts[0]); return 1; }
    REFUSED(frt_scene_set_mesh_morph_weights(s, 0, weights, 2, 0), "a mesh without targets took weights");
    REFUSED(frt_scene_set_mesh_morph_targets(s, 0, deltas, 4, 0), "no targets were taken");
    REFUSED(frt_scene_set_mesh_morph_targets(s, 0, deltas, 4, FRT_MAX_MORPH_TARGETS + 1u), "too many targets were taken");
    REFUSED(frt_scene_set_mesh_morph_targets(s, 0, deltas, 3, 2), "a wrong vertex count was taken");
    CHECK(frt_scene_set_mesh_morph_targets(s, 0, deltas, 4, 2));
    CHECK(frt_scene_set_mesh_morph_weights(s, 0, weights, 2, FRT_DEFORM_RECOMPUTE_NORMALS));
    CHECK(frt_scene_get(s, 0, tris));                       /* per triangle v0, e1, e2: vertex 0 stays, vertices 2 and 3 rise by 0.5 */
    if (tris[1] != 0.0f || tris[3 + 1] != 0.5f || tris[6 + 1] != 0.0f || tris[9 + 3 + 1] != 0.5f || tris[9 + 6 + 1] != 0.5f) {
        fprintf(stderr, "morphed heights: %g %g %g %g %g\n", tris[1], tris[4], tris[7], tris[13], tris[16]);
        return 1;
    }
    CHECK(frt_scene_set_mesh_morph_weights(s, 0, above, 2, 0));          /* from the base again, not from the last morph */
    CHECK(frt_scene_get(s, 0, tris));
    if (tris[3 + 1] != 1.5f || tris[9 + 3 + 1] != 0.75f) { fprintf(stderr, "second morph: %g %g\n", tris[4], tris[13]); return 1; }
    REFUSED(frt_scene_set_mesh_morph_weights(s, 0, weights, 3, 0), "a wrong target count was taken");
    REFUSED(frt_scene_set_mesh_morph_weights(s, 0, bad, 2, 0), "a non-finite weight was taken");
    REFUSED(frt_scene_set_mesh_morph_weights(s, 0, weights, 2, FRT_DEFORM_DEVICE), "a scene took device weights");
    /* morph, then skin: joint 1 (vertices 2 and 3) moves up by 0.25 */
    memcpy(mats, identity, sizeof(identity));
    memcpy(mats + 16, identity, sizeof(identity));
    mats[16 + 13] = 0.25f;
    REFUSED(frt_scene_set_mesh_pose_ex(s, 0, mats, 2, weights, 2, 0), "a mesh without a skin took a pose");
    CHECK(frt_scene_set_mesh_skin(s, 0, joints, skin_w, 4, 2));
    CHECK(frt_scene_set_mesh_pose_ex(s, 0, mats, 2, weights, 2, 0));
    CHECK(frt_scene_get(s, 0, tris));
    if (tris[1] != 0.0f || tris[3 + 1] != 0.75f || tris[9 + 3 + 1] != 0.75f) { fprintf(stderr, "morphed and posed: %g %g %g\n", tris[1], tris[4], tris[13]); return 1; }
    REFUSED(frt_scene_set_mesh_pose_ex(s, 0, mats, 2, weights, 1, 0), "the combined call took a wrong target count");

    if (gpu) {      /* the same on a renderer's replica */
        frt_render_opts opts;
        frt_renderer* r;
        unsigned char slots_host[2 * 48], slots_dev[2 * 48];
        uint32_t rejects = 7;
        if (frt_device_count() < 1) { fprintf(stderr, "no HIP device\n"); return 1; }
        /* the scene back at rest, both bindings made again there, so scene and replica start alike */
        CHECK(frt_scene_set_mesh_morph_targets(s, 0, NULL, 0, 0));
        CHECK(frt_scene_set_mesh_skin(s, 0, NULL, NULL, 0, 0));
        CHECK(frt_scene_set_mesh_vertices(s, 0, pos, NULL, 4));
        memset(&opts, 0, sizeof(opts));
        opts.max_depth = 2;
        r = frt_renderer_create(s, 32, 24, &opts);
        if (!r) { fprintf(stderr, "renderer: %s\n", frt_last_error()); return 1; }
        REFUSED(frt_renderer_set_mesh_morph_weights(r, 0, weights, 2, 0), "a replica without targets took weights");
        CHECK(frt_scene_set_mesh_morph_targets(s, 0, deltas, 4, 2));
        CHECK(frt_renderer_set_mesh_morph_targets(r, 0, deltas, 4, 2));
        CHECK(frt_scene_set_mesh_skin(s, 0, joints, skin_w, 4, 2));
        CHECK(frt_renderer_set_mesh_skin(r, 0, joints, skin_w, 4, 2));
        CHECK(frt_scene_set_mesh_morph_weights(s, 0, weights, 2, FRT_DEFORM_RECOMPUTE_NORMALS));
        CHECK(frt_renderer_set_mesh_morph_weights(r, 0, weights, 2, FRT_DEFORM_RECOMPUTE_NORMALS));
        CHECK(frt_renderer_read_scene(r, 13, slots_dev));
        CHECK(frt_scene_get(s, 13, slots_host));
        if (memcmp(slots_host, slots_dev, sizeof(slots_host)) != 0) { fprintf(stderr, "the morphed replica differs from the morphed scene\n"); return 1; }
        CHECK(frt_scene_set_mesh_pose_ex(s, 0, mats, 2, above, 2, 0));
        CHECK(frt_renderer_set_mesh_pose_ex(r, 0, mats, 2, above, 2, 0));
        CHECK(frt_renderer_read_scene(r, 13, slots_dev));
        CHECK(frt_scene_get(s, 13, slots_host));
        if (memcmp(slots_host, slots_dev, sizeof(slots_host)) != 0) { fprintf(stderr, "the morphed and posed replica differs from the scene\n"); return 1; }
        REFUSED(frt_renderer_set_mesh_morph_weights(r, 0, bad, 2, 0), "a renderer took a non-finite host weight");
        CHECK(frt_renderer_deform_rejects(r, &rejects));
        if (rejects != 0) { fprintf(stderr, "%u rejects\n", rejects); return 1; }
        CHECK(frt_renderer_set_mesh_morph_targets(r, 0, NULL, 0, 0));
        REFUSED(frt_renderer_set_mesh_morph_weights(r, 0, weights, 2, 0), "the targets did not leave the replica");
        frt_renderer_destroy(r);
    }
    CHECK(frt_scene_set_mesh_morph_targets(s, 0, NULL, 0, 0));
    REFUSED(frt_scene_set_mesh_morph_weights(s, 0, weights, 2, 0), "the targets did not leave");
    frt_scene_destroy(s);
    printf(gpu ? "morph ok (gpu)\n" : "morph ok\n");
    return 0;
}
