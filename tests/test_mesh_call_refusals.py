"""The order of refusals of the seven mesh-edit calls of a scene (include/frt.h: frt_scene_set_mesh_vertices, _set_mesh_vertices_ex, _set_mesh_skin,
_set_mesh_pose, _set_mesh_pose_ex, _set_mesh_morph_targets, _set_mesh_morph_weights): every row of tests/_mesh_calls.py is
wrong in two or more ways at once, and the call names exactly one of them — the code and the message below, recorded before the family's checks were
gathered into one preamble, so that the order (not built, the device flag, unknown flag bits, the mesh id, then the arguments in each call's own
order) cannot move unnoticed. Nothing of a refused call is applied."""
import pytest
from _mesh_calls import pose_scene, bind_for_refusals, refusal_rows, run_row

EXPECT = {
    'not built, vertices: bad id':
        (-4, 'set_mesh_vertices: scene is not built'),
    'not built, vertices_ex: bad id, device flag':
        (-4, 'set_mesh_vertices: scene is not built'),
    'not built, skin: bad id':
        (-4, 'set_mesh_skin: scene is not built'),
    'not built, pose: bad id, unknown bit':
        (-4, 'set_mesh_pose: scene is not built'),
    'not built, pose_ex: bad id, NaN weight':
        (-4, 'set_mesh_pose: scene is not built'),
    'not built, targets: bad id':
        (-4, 'set_mesh_morph_targets: scene is not built'),
    'not built, weights: bad id, device flag':
        (-4, 'set_mesh_morph_weights: scene is not built'),
    'vertices: bad id, null positions':
        (-1, 'set_mesh_vertices: mesh id 99 out of range (3 meshes)'),
    'vertices: wrong count, NaN position':
        (-1, 'set_mesh_vertices: 5 vertices given, the mesh has 4 (the topology is fixed)'),
    'vertices: null positions, wrong count':
        (-1, 'set_mesh_vertices: null positions'),
    'vertices: NaN position, NaN attributes':
        (-1, 'set_mesh_vertices: position of vertex 3 is not finite'),
    'vertices_ex: device flag, unknown bit':
        (-1, 'set_mesh_vertices: FRT_DEFORM_DEVICE is for frt_renderer_set_mesh_vertices_ex only (a scene lives in host memory)'),
    'vertices_ex: unknown bit, bad id':
        (-1, 'set_mesh_vertices: unknown flag bits'),
    'vertices_ex: device flag, bad id':
        (-1, 'set_mesh_vertices: FRT_DEFORM_DEVICE is for frt_renderer_set_mesh_vertices_ex only (a scene lives in host memory)'),
    'vertices_ex: bad id, null positions':
        (-1, 'set_mesh_vertices: mesh id 99 out of range (3 meshes)'),
    'vertices_ex: wrong count, NaN position':
        (-1, 'set_mesh_vertices: 5 vertices given, the mesh has 4 (the topology is fixed)'),
    'skin: bad id, null joints':
        (-1, 'set_mesh_skin: mesh id 99 out of range (3 meshes)'),
    'skin: bad id, null weights':
        (-1, 'set_mesh_skin: mesh id 99 out of range (3 meshes)'),
    'skin: null weights, wrong count':
        (-1, 'set_mesh_skin: null joints or weights'),
    'skin: wrong count, NaN weight':
        (-1, 'set_mesh_skin: 5 vertices given, the mesh has 4'),
    'skin: no joints, a joint out of range':
        (-1, 'set_mesh_skin: 0 joints (1 to 65536: a joint index is 16 bits)'),
    'skin: a joint out of range, a negative weight':
        (-1, 'set_mesh_skin: vertex 0 names joint 1 of 1'),
    'pose: device flag, unknown bit':
        (-1, 'set_mesh_pose: FRT_DEFORM_DEVICE is for frt_renderer_set_mesh_pose only (a scene lives in host memory)'),
    'pose: unknown bit, bad id':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose: device flag, bad id':
        (-1, 'set_mesh_pose: FRT_DEFORM_DEVICE is for frt_renderer_set_mesh_pose only (a scene lives in host memory)'),
    'pose: bad id, null palette':
        (-1, 'set_mesh_pose: mesh id 99 out of range (3 meshes)'),
    'pose: wrong count, NaN entry':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'pose: wrong count, null palette':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'pose: no skin, wrong count':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose: no skin, null palette':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose_ex: device flag, unknown bit':
        (-1, 'set_mesh_pose: FRT_DEFORM_DEVICE is for frt_renderer_set_mesh_pose only (a scene lives in host memory)'),
    'pose_ex: unknown bit, bad id':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose_ex: unknown bit, bad id, no weights':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose_ex: bad id, null palette, null weights':
        (-1, 'set_mesh_pose: mesh id 99 out of range (3 meshes)'),
    'pose_ex: no skin, no targets':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose_ex: no skin, wrong count, no weights':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose_ex: NaN palette, NaN weight':
        (-1, 'set_mesh_pose: joint matrix 0 has a non-finite entry'),
    'pose_ex: wrong palette count, wrong weight count':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'pose_ex: null palette, null weights':
        (-1, 'set_mesh_pose: null joint matrices'),
    'pose_ex: wrong weight count, NaN weight':
        (-1, 'set_mesh_pose: 3 weights given, 2 targets are bound'),
    'pose_ex: null weights with a count':
        (-1, 'set_mesh_pose: null weights'),
    'pose_ex: weights with no count':
        (-1, 'set_mesh_pose: 0 weights given, 2 targets are bound'),
    'targets: bad id, null deltas':
        (-1, 'set_mesh_morph_targets: mesh id 99 out of range (3 meshes)'),
    'targets: bad id, no targets':
        (-1, 'set_mesh_morph_targets: mesh id 99 out of range (3 meshes)'),
    'targets: wrong count, NaN delta':
        (-1, 'set_mesh_morph_targets: 5 vertices given, the mesh has 4'),
    'targets: no targets, NaN delta':
        (-1, 'set_mesh_morph_targets: 0 targets (1 to 4096)'),
    'targets: too many targets, NaN delta':
        (-1, 'set_mesh_morph_targets: 4097 targets (1 to 4096)'),
    'weights: device flag, unknown bit':
        (-1, 'set_mesh_morph_weights: FRT_DEFORM_DEVICE is for frt_renderer_set_mesh_morph_weights only (a scene lives in host memory)'),
    'weights: unknown bit, bad id':
        (-1, 'set_mesh_morph_weights: unknown flag bits'),
    'weights: device flag, bad id':
        (-1, 'set_mesh_morph_weights: FRT_DEFORM_DEVICE is for frt_renderer_set_mesh_morph_weights only (a scene lives in host memory)'),
    'weights: bad id, null weights':
        (-1, 'set_mesh_morph_weights: mesh id 99 out of range (3 meshes)'),
    'weights: wrong count, NaN weight':
        (-1, 'set_mesh_morph_weights: 3 weights given, 2 targets are bound'),
    'weights: wrong count, null weights':
        (-1, 'set_mesh_morph_weights: 3 weights given, 2 targets are bound'),
    'weights: no targets, wrong count':
        (-1, 'set_mesh_morph_weights: the mesh has no morph targets (set_mesh_morph_targets)'),
    'weights: no targets, null weights':
        (-1, 'set_mesh_morph_weights: the mesh has no morph targets (set_mesh_morph_targets)'),
}


@pytest.fixture(scope="module")
def scenes(frt):
    built, _ = pose_scene(frt)
    bind_for_refusals(built)
    unbuilt, _ = pose_scene(frt, build=False)
    return built, unbuilt


def test_the_table_covers_every_call_and_every_pair(frt):
    rows = refusal_rows(frt, "scene")
    assert [rid for rid, _, _ in rows] == list(EXPECT)
    calls = {"set_mesh_vertices", "set_mesh_vertices_ex", "set_mesh_skin", "set_mesh_pose", "set_mesh_pose_ex", "set_mesh_morph_targets", "set_mesh_morph_weights"}
    assert {c for _, c, _ in rows} == calls
    assert {c for rid, c, _ in rows if rid.startswith("not built")} == calls and {c for rid, c, _ in rows if "bad id, null" in rid} == calls
    for pair in ("device flag, unknown bit", "unknown bit, bad id", "wrong count, NaN", "no skin, wrong count", "no targets, wrong count", "NaN palette, NaN weight"):
        assert any(pair in rid for rid in EXPECT), pair


@pytest.mark.parametrize("rid", list(EXPECT))
def test_refusal(frt, scenes, rid):
    built, unbuilt = scenes
    call, args = {r: (c, a) for r, c, a in refusal_rows(frt, "scene")}[rid]
    before = {w: built.get(w).tobytes() for w in ("tris", "attributes", "shade_tris")}
    got = run_row(frt, "frt_scene_", (unbuilt if rid.startswith("not built") else built)._h, call, args)
    assert got == EXPECT[rid]
    assert {w: built.get(w).tobytes() for w in before} == before
