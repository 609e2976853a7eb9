"""The rig of a glTF document through the loader (include/frt.h: frt_model_rig_counts and the calls after it; DESIGN.md section 11, "Animation"): a
two-primitive character loads to the arrays it was written from, value for value; nodes are stored parents first with the index mapping kept; a skin
without inverseBindMatrices gets identities; Model.rig equals a frt.Rig built from those arrays; the documents that have to be refused are; and a
document of the existing kind loads as before."""
import json
import numpy as np
import pytest
from _gltf_rig import F, RigWriter, character
from test_loader import _sphere_model, _check_model


def same(a, b):
    return np.ascontiguousarray(a, F).view(np.uint32).tolist() == np.ascontiguousarray(b, F).view(np.uint32).tolist()


@pytest.mark.parametrize("kind", ["gltf", "glb"])
def test_character_loads_value_for_value(frt, tmp_path, kind):
    w, ref = character()
    path = tmp_path / ("character." + kind)
    w.save_gltf(str(path)) if kind == "gltf" else w.save_glb(str(path))
    m = frt.loader.load_gltf(path)
    assert m.counts()["geometries"] == 2 and m.warnings() == [] and m.rig_counts() == {"nodes": 6, "skins": 2, "animations": 2}
    for g in range(2):
        geo, _ = m.geometry(g)
        assert same(geo.positions[:, :3], ref["pos"][g]) and geo.indices.tolist() == ref["idx"][g].tolist()
        j, wt, skin = m.skin(g)
        assert j.dtype == np.uint16 and j.tolist() == ref["joints"][g].tolist() and same(wt, ref["weights"][g]) and skin == 0
        d, dw = m.morph_targets(g)
        assert d.shape == (2, len(ref["pos"][g]), 3) and same(d, ref["deltas"][g]) and same(dw, ref["default_weights"])
    n = m.nodes()
    assert n["document_index"].tolist() == ref["order"] and n["parents"].tolist() == ref["parents"].tolist()      # parents first, mapping kept
    assert all(p < i for i, p in enumerate(n["parents"]))
    for k in ("translations", "rotations", "scales"):
        assert same(n[k], ref[k]), k
    assert n["has_matrix"].tolist() == ref["has_matrix"].tolist() and same(n["matrices"][3], ref["matrix"])
    j, ib = m.skin_joints(0)
    assert j.tolist() == ref["skin_joints"].tolist() and same(ib, ref["inverse_bind"])
    j, ib = m.skin_joints(1)                                                                                         # no inverseBindMatrices
    assert j.tolist() == ref["skin_joints"].tolist() and np.array_equal(ib, np.tile(np.eye(4, dtype=F).reshape(16), (5, 1)))
    got = m.animations()
    assert [a[0] for a in got] == ["wave", "nod"]
    for (_, gc), (_, rc) in zip(got, ref["animations"]):
        assert len(gc) == len(rc)
        for a, b in zip(gc, rc):
            assert (a["node"], a["path"], a["interpolation"]) == (b["node"], b["path"], b["interpolation"])
            assert same(a["times"], b["times"]) and a["values"].shape == b["values"].shape and same(a["values"], b["values"]), b["path"]


def test_model_rig_is_the_rig_of_the_arrays(frt, tmp_path):
    w, ref = character()
    path = tmp_path / "character.gltf"
    w.save_gltf(str(path))
    m = frt.loader.load_gltf(path)
    n = m.nodes()
    joints, ib = m.skin_joints(0)
    by_hand = frt.Rig(n["parents"], n["translations"], n["rotations"], n["scales"], matrices={3: n["matrices"][3]}, joint_nodes=joints, inverse_bind=ib,
                      num_targets=2, default_weights=ref["default_weights"], clips=m.animations())
    rig = m.rig(0)
    assert (rig.num_nodes, rig.num_joints, rig.num_targets) == (6, 5, 2) and rig.clips == by_hand.clips == [("wave", 1.25), ("nod", 1.25)]
    for clip in ("wave", "nod"):
        for t in (-1.0, 0.0, 0.3, 0.5, 0.9, 1.25, 2.0):
            a, b = rig.evaluate(clip, t), by_hand.evaluate(clip, t)
            assert same(a[0], b[0]) and same(a[1], b[1]), (clip, t)
    assert not same(rig.evaluate("wave", 0.3)[0], rig.evaluate("wave", 0.9)[0])
    bare = frt.Rig.from_model(m, 1)                      # the skin without inverse binds
    assert bare.num_joints == 5
    morph = m.rig(None)
    assert (morph.num_joints, morph.num_targets) == (0, 2) and same(morph.evaluate("wave", 0.5)[1], rig.evaluate("wave", 0.5)[1])
    with pytest.raises(frt.FrtError):
        m.rig(2)


def test_bind_character_binds_every_geometry(frt, tmp_path):
    w, ref = character()
    path = tmp_path / "character.glb"
    w.save_glb(str(path))
    m = frt.loader.load_gltf(path)
    b = frt.SceneBuilder()
    ids = [b.add_mesh(m.geometry(g)[0]) for g in range(2)]
    mat = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    for i in ids:
        b.add_instance(i, mat, np.eye(4, dtype=F))
    b.add_mesh(frt.geometry.create_plane())
    b.register_quad_light(2, np.eye(4, dtype=F), (1.0, 1.0, 1.0), 5.0)
    scene = b.build()
    before = scene.get("tri_slots").tobytes()
    assert frt.loader.bind_character(scene, m, ids) == ids
    rig = m.rig(0)
    scene.animate(rig, ids, "wave", 0.4)
    assert scene.get("tri_slots").tobytes() != before


def _refused(frt, tmp_path, edit, match):
    w, _ = character()
    edit(w)
    path = tmp_path / "bad.gltf"
    w.save_gltf(str(path))
    with pytest.raises(frt.FrtError, match=match):
        frt.loader.load_gltf(path)


def test_refusals(frt, tmp_path):
    def cycle(w):
        w.doc["nodes"][2]["children"] = [3]              # 3 -> 1 -> 2 -> 3

    def two_parents(w):
        w.doc["nodes"][0]["children"] = [5]

    def joint_not_a_node(w):
        w.doc["skins"][1]["joints"][2] = 6

    def times_not_increasing(w):
        s = w.doc["animations"][0]["samplers"][0]
        s["input"] = w.accessor(F([0.0, 0.5, 0.5]))

    def times_not_finite(w):
        s = w.doc["animations"][1]["samplers"][0]
        s["input"] = w.accessor(F([0.0, np.inf]))

    def output_count(w):
        s = w.doc["animations"][0]["samplers"][0]      # LINEAR translation, 3 keys
        s["output"] = w.accessor(np.zeros((2, 3), F))

    def cubic_output_count(w):
        s = w.doc["animations"][0]["samplers"][1]      # CUBICSPLINE rotation, 3 keys: 9 rows
        s["output"] = w.accessor(np.zeros((3, 4), F))

    for edit, match in ((cycle, "cycle"), (two_parents, "cycle or a node with two parents"), (joint_not_a_node, "joint that is not a node"),
                        (times_not_increasing, "strictly increasing"), (times_not_finite, "strictly increasing"), (output_count, "output has"),
                        (cubic_output_count, "output has")):
        _refused(frt, tmp_path, edit, match)


def test_unsupported_parts_warn_and_are_skipped(frt, tmp_path):
    w, ref = character()
    prim = w.doc["meshes"][0]["primitives"][0]
    prim["attributes"]["JOINTS_1"] = prim["attributes"]["JOINTS_0"]
    prim["attributes"]["WEIGHTS_1"] = prim["attributes"]["WEIGHTS_0"]
    a = w.doc["animations"][0]
    a["channels"].append({"sampler": 0, "target": {"node": 4, "path": "translation"}})      # a channel on the matrix node
    a["channels"].append({"sampler": 0, "target": {"node": 1, "path": "pointer"}})
    path = tmp_path / "extra.gltf"
    w.save_gltf(str(path))
    m = frt.loader.load_gltf(path)
    ws = m.warnings()
    assert len(ws) == 3 and "JOINTS_1" in ws[0] and "matrix" in ws[1] and "skipped" in ws[2]
    assert m.skin(0)[0].tolist() == ref["joints"][0].tolist() and len(m.animations()[0][1]) == 3


@pytest.mark.parametrize("kind", ["glb", "gltf"])
def test_a_document_of_the_existing_kind_loads_as_before(frt, tmp_path, kind):
    path, ref = _sphere_model(tmp_path, frt, kind=kind)
    m = frt.loader.load_gltf(path)
    _check_model(frt, m, ref)                            # the same geometries, three of them, and no warning
    assert m.warnings() == [] and m.rig_counts() == {"nodes": 0, "skins": 0, "animations": 0}
    assert all(m.skin(g) is None and m.morph_targets(g) is None for g in range(3))
    with pytest.raises(frt.FrtError):
        m.rig(0)
    with pytest.raises(frt.FrtError):
        m.rig(None)
    assert json.loads(RigWriter().json())["asset"]["version"] == "2.0"
