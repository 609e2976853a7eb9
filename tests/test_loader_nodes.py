"""Node animation through the loader (include/frt.h: frt_model_geometry_nodes, frt_rig_from_model_nodes; DESIGN.md section 11, "Node animation"): a
document in which nothing is skinned (a root, two children that carry two meshes, a rotation and a translation channel) tells which stored node carries
which geometry and becomes a nodes-only rig equal to one built by hand; a document with a skin loads as before."""
import numpy as np
import pytest
from _gltf_rig import F, RigWriter, character, unit


def same(a, b):
    return np.ascontiguousarray(a, F).view(np.uint32).tolist() == np.ascontiguousarray(b, F).view(np.uint32).tolist()


def gear_train(tmp_path):
    """Document nodes 0 and 1 (children of 2, written in front of it: not parents first) carry meshes 0 and 1; node 0 has a rotation channel, node 1 a
    translation channel; no skin."""
    rng = np.random.default_rng(3)
    w = RigWriter()
    for nverts in (4, 3):
        pos = rng.uniform(-0.3, 0.3, (nverts, 3)).astype(F)
        idx = np.array([0, 1, 2, 1, 3, 2] if nverts == 4 else [0, 1, 2], np.uint16)
        w.doc["meshes"].append({"primitives": [{"attributes": {"POSITION": w.accessor(pos)}, "indices": w.accessor(idx)}]})
    w.doc["nodes"] = [{"mesh": 0, "translation": [0.5, 0.0, 0.0], "rotation": unit([0.1, 0.2, 0.3, 0.9]).tolist()},
                      {"mesh": 1, "translation": [-0.5, 0.25, 0.0], "scale": [1.5, 1.5, 1.5]},
                      {"children": [0, 1], "translation": [0.0, 1.0, -2.0], "rotation": unit([0.0, 0.3, 0.0, 0.95]).tolist()}]
    t3, t2 = F([0.0, 0.5, 1.25]), F([0.25, 1.0])
    turn = unit(rng.standard_normal((3, 4)))
    slide = (0.2 * rng.standard_normal((2, 3))).astype(F)
    a = {"name": "run", "channels": []}
    a["channels"] = [{"sampler": w.sampler(a, t3, w.accessor(turn), "LINEAR"), "target": {"node": 0, "path": "rotation"}},
                     {"sampler": w.sampler(a, t2, w.accessor(slide), "LINEAR"), "target": {"node": 1, "path": "translation"}}]
    w.doc["animations"] = [a]
    path = tmp_path / "gears.glb"
    w.save_glb(str(path))
    return path


def test_geometry_nodes_and_the_node_rig(frt, tmp_path):
    m = frt.loader.load_gltf(gear_train(tmp_path))
    assert m.counts()["geometries"] == 2 and m.rig_counts() == {"nodes": 3, "skins": 0, "animations": 1}
    n = m.nodes()
    stored = {int(d): i for i, d in enumerate(n["document_index"])}
    assert n["parents"][stored[2]] == -1 and stored[2] == 0      # parents first: the root, written last, is stored first
    for geo, doc_node in ((0, 0), (1, 1)):
        got = m.geometry_nodes(geo)
        assert got.dtype == np.uint32 and got.tolist() == [stored[doc_node]]
    with pytest.raises(frt.FrtError):
        m.geometry_nodes(2)
    with pytest.raises(frt.FrtError):      # neither joints nor targets: no rig for meshes
        m.rig(None)
    rig = m.node_rig()
    assert (rig.num_nodes, rig.num_joints, rig.num_targets) == (3, 0, 0) and rig.clips == [("run", 1.25)]
    by_hand = frt.Rig(n["parents"], n["translations"], n["rotations"], n["scales"], clips=m.animations(), nodes_only=True)
    nodes = [int(m.geometry_nodes(g)[0]) for g in range(2)]
    root = np.eye(4, dtype=F).reshape(16) * F(0.5)
    for t in (-1.0, 0.0, 0.3, 0.5, 0.9, 1.25, 2.0):
        for kw in ({}, {"root": root}):
            assert same(rig.evaluate_nodes("run", t, nodes, **kw), by_hand.evaluate_nodes("run", t, nodes, **kw)), t
    assert not same(rig.evaluate_nodes("run", 0.3, nodes), rig.evaluate_nodes("run", 0.9, nodes))


def test_a_document_with_a_skin_loads_as_before(frt, tmp_path):
    w, ref = character()
    path = tmp_path / "character.glb"
    w.save_glb(str(path))
    m = frt.loader.load_gltf(path)
    assert m.counts()["geometries"] == 2 and m.warnings() == [] and m.rig_counts() == {"nodes": 6, "skins": 2, "animations": 2}
    for g in range(2):
        geo, _ = m.geometry(g)
        assert same(geo.positions[:, :3], ref["pos"][g]) and geo.indices.tolist() == ref["idx"][g].tolist()
        assert m.geometry_nodes(g).tolist() == [0]      # both primitives are of the mesh on stored node 0
    rig, nodes_only = m.rig(0), m.node_rig()
    assert (rig.num_joints, rig.num_targets) == (5, 2) and (nodes_only.num_joints, nodes_only.num_targets, nodes_only.num_clips) == (0, 0, 2)
    joints, ib = m.skin_joints(0)
    for clip, t in (("wave", 0.3), ("nod", 0.8)):      # the weights channel is left out, the node channels are the skinned rig's
        assert same(nodes_only.evaluate_nodes(clip, t, joints, offsets=ib), rig.evaluate(clip, t)[0])


def test_an_obj_model_has_no_nodes(frt, tmp_path):
    path = tmp_path / "tri.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\n")
    m = frt.loader.load_gltf(path)
    assert m.counts()["geometries"] == 1 and m.geometry_nodes(0).size == 0
    with pytest.raises(frt.FrtError):
        m.node_rig()
