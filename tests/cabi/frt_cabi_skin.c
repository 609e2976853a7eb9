/* Skinning from plain C (include/frt.h: frt_scene_set_mesh_skin, frt_scene_set_mesh_pose): a one-quad scene is built, two joints are bound to its four
 * vertices, and a pose that moves joint 1 up by 0.5 leaves the world-space triangles where the contract puts them. Host calls only: runs without a device.
 *   gcc -std=c99 -I include tests/cabi/frt_cabi_skin.c -L fast-raytracing-wgpu_amd/lib -lfrt */
#include "frt.h"
#include <stdio.h>
#include <string.h>

#define CHECK(call) do { int rc_ = (call); if (rc_ < 0) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, frt_last_error()); return 1; } } while (0)

int main(void) {
    const float pos[16] = {-1, 0, -1, 1,   1, 0, -1, 1,   1, 0, 1, 1,   -1, 0, 1, 1};
    const uint32_t idx[6] = {0, 2, 1, 0, 3, 2};
    const float white[4] = {1, 1, 1, 1};
    const float identity[16] = {1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1};
    frt_vertex_attr attrs[4];
    frt_material mat;
    uint32_t counts[8];
    float tris[2 * 9], mats[32];
    /* vertices 0 and 1 follow joint 0, vertex 2 joint 1, vertex 3 both halfway; every slot is evaluated, the weight-0 ones too */
    const uint16_t joints[16] = {0, 0, 0, 0,   0, 1, 0, 0,   1, 1, 1, 1,   0, 1, 0, 1};
    const float weights[16] = {1, 0, 0, 0,   1, 0, 0, 0,   0.25f, 0.25f, 0.25f, 0.25f,   0.5f, 0.5f, 0, 0};
    frt_scene* s = frt_scene_create();
    if (!s) { fprintf(stderr, "scene: %s\n", frt_last_error()); return 1; }
    memset(attrs, 0, sizeof(attrs));
    frt_material_default(white, &mat);
    CHECK(frt_scene_add_mesh(s, pos, 4, attrs, idx, 6));
    CHECK(frt_scene_add_material(s, &mat));
    if (frt_scene_set_mesh_skin(s, 0, joints, weights, 4, 2) != FRT_ERR_STATE) { fprintf(stderr, "an unbuilt scene took a skin\n"); return 1; }
    CHECK(frt_scene_add_instance(s, 0, 0, identity));
    CHECK(frt_scene_build(s));
    CHECK(frt_scene_counts(s, counts));
    if (counts[0] != 2) { fprintf(stderr, "%u triangles\n", counts[0]); return 1; }
    memcpy(mats, identity, sizeof(identity));
    memcpy(mats + 16, identity, sizeof(identity));
    mats[16 + 13] = 0.5f;                                   /* joint 1: up by one half */
    if (frt_scene_set_mesh_pose(s, 0, mats, 2, 0) != FRT_ERR_INVALID_ARG) { fprintf(stderr, "a mesh without a skin took a pose\n"); return 1; }
    CHECK(frt_scene_set_mesh_skin(s, 0, joints, weights, 4, 2));
    CHECK(frt_scene_set_mesh_pose(s, 0, mats, 2, FRT_DEFORM_RECOMPUTE_NORMALS));
    CHECK(frt_scene_get(s, 0, tris));                       /* per triangle v0, e1, e2: vertex 0 stays, vertex 2 rises by 0.5, vertex 3 by 0.25 */
    if (tris[1] != 0.0f || tris[3 + 1] != 0.5f || tris[6 + 1] != 0.0f || tris[9 + 3 + 1] != 0.25f || tris[9 + 6 + 1] != 0.5f) {
        fprintf(stderr, "posed heights: %g %g %g %g %g\n", tris[1], tris[4], tris[7], tris[13], tris[16]);
        return 1;
    }
    if (frt_scene_set_mesh_pose(s, 0, mats, 3, 0) != FRT_ERR_INVALID_ARG) { fprintf(stderr, "a wrong joint count was taken\n"); return 1; }
    CHECK(frt_scene_set_mesh_skin(s, 0, NULL, NULL, 0, 0));
    if (frt_scene_set_mesh_pose(s, 0, mats, 2, 0) != FRT_ERR_INVALID_ARG) { fprintf(stderr, "the skin did not leave\n"); return 1; }
    frt_scene_destroy(s);
    printf("skin ok\n");
    return 0;
}
