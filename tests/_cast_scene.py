"""What the animate_cast tests share (include/frt.h: frt_renderer_animate_cast; DESIGN.md section 11, "Animating a cast"): one host scene with a cast
on it, and the cast itself — three characters with different rigs and two node-animated sets of instances — bound to anything that has the bind
calls of a renderer, or handed to a host scene entry by entry.

The scene is the Cornell Box (meshes 0 .. 3, instances 0 .. 8) and
  instances 9 .. 301: 293 small planes (mesh 0), so that one instance binding has 300 instances, past the 256-lane stride of the kernel's last phase;
  meshes 4 .. 9 with one instance each (302 .. 307): four more planes of 4 vertices, a sphere and a crystal, the characters' meshes;
  mesh 10, a plane no instance uses (a binding on it can be removed with its mesh).
A wave of the segmented pose kernels holds 64 consecutive vertices of the call's concatenation: with planes of 4 vertices next to each other in it,
one wave holds vertices of all three characters, each under a palette and weights of its own."""
import numpy as np
from test_mesh_deform import PLANE, SPHERE, CRYSTAL_MESH
from test_instance_update import cornell_meshes
from _skin_model import make_skin
from _morph_model import make_targets
from _anim_model import F, make_rig, sample_times

TALL_BOX = 8
CROWD = 293
FIRST_CHARACTER_MESH = 4
CHARACTER_MESHES = (PLANE, PLANE, PLANE, PLANE, SPHERE, CRYSTAL_MESH)      # the geometry of meshes 4 .. 9
SPARE_MESH = 10
FIRST_CHARACTER_INSTANCE = 9 + CROWD


def cast_scene(frt):
    """(host scene, the geometry of every mesh)."""
    ref = frt.scenes.create_cornell_box()
    inst, mats = ref.get("instances"), ref.get("materials")
    geo = cornell_meshes(frt)
    geo = geo + [geo[m] for m in CHARACTER_MESHES] + [geo[PLANE]]
    b = frt.SceneBuilder()
    for g in geo:
        b.add_mesh(g)
    for k in range(6):
        b.add_material(frt.Material.from_buffer_copy(np.ascontiguousarray(mats[k]).tobytes()))
    for k, row in enumerate(inst):
        m = row[5:21].view(F)
        if k == 5:      # (the factory's order: 5 the quad light, 7 the sphere light)
            b.register_quad_light(int(row[0]), m, (1.0, 1.0, 1.0), 10.0)
        elif k == 7:
            b.register_sphere_light(int(row[0]), m, (0.02, 0.02, 0.9), 10.0)
        else:
            b.add_instance(int(row[0]), int(row[1]), m)
    rng = np.random.default_rng(11)
    small = np.tile(np.eye(4, dtype=F).reshape(16), (CROWD + len(CHARACTER_MESHES), 1))
    small[:, [0, 5, 10]] = F(0.02)
    small[CROWD:, [0, 5, 10]] = F(0.15)
    small[:, 12:15] = rng.uniform(-0.8, 0.8, (len(small), 3)).astype(F)
    for k in range(CROWD):
        b.add_instance(PLANE, 0, small[k])
    for k in range(len(CHARACTER_MESHES)):
        b.add_instance(FIRST_CHARACTER_MESH + k, 1 + k % 4, small[CROWD + k])
    fs = b.build()
    assert fs.counts()["instances"] == FIRST_CHARACTER_INSTANCE + len(CHARACTER_MESHES)
    return fs, geo


def near_identity(rng, n, spread=0.1):
    m = np.tile(np.eye(4, dtype=F).reshape(16), (n, 1))
    m[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] += (spread * rng.standard_normal((n, 9))).astype(F)
    m[:, 12:15] = (spread * rng.standard_normal((n, 3))).astype(F)
    return m


def three_times(desc):
    t = sample_times(desc, 9)      # before the clip, a key time, between keys
    return F([t[0], t[4], t[8]])


def tame(desc, scale=0.2):
    """The rig moved towards the origin, so that what hangs on it stays about the box."""
    desc["translations"] = F(scale) * desc["translations"]
    for ch in desc["clips"][0][1]:
        if ch["path"] == "translation":
            ch["values"] = F(scale) * ch["values"]
    return desc


def burst_clip():
    """A clip under which the second node's global translation overflows: 3e38 on the root, doubled by its child."""
    far = F([[0, 0, 0], [3e38, 0, 0]])
    return ("burst", [{"node": n, "path": "translation", "interpolation": "LINEAR", "times": F([0.0, 1.0]), "values": far} for n in (0, 1)])


def vanish_clip(node):
    return ("vanish", [{"node": node, "path": "scale", "interpolation": "LINEAR", "times": F([0.0, 1.0]), "values": F([[1, 1, 1], [0, 0, 0]])}])


class Cast:
    """The descriptions and rigs of the cast. Members, by name:
      "chain2":  a character, J = 2, T = 0, meshes 4 and 5 (planes); with the clip "burst"
      "tree257": a character, every node a joint, T = 3, meshes 6 (a plane) and 8 (the sphere)
      "morph":   a morph-only character, J = 0, T = 2, meshes 7 (a plane) and 9 (the crystal)
      "crowd":   300 instances (all of 0 .. 301 but 7 and 8, permuted) on the nodes of a 12-node rig, with root and offsets
      "pair":    instances 8 and 7 on nodes 3 and 0 of the same rig, with neither; with the clip "vanish" (node 3 scaled to zero)
      "spare":   a character as "chain2" on mesh 10, which has no instance"""
    MESHES = {"chain2": [4, 5], "tree257": [6, 8], "morph": [7, 9], "spare": [SPARE_MESH]}

    def __init__(self, frt):
        self.frt = frt
        self.desc, self.rig, self.kw = {}, {}, {}
        chain2 = make_rig("chain2", joints="all", num_targets=0, keys=(2, 5))
        chain2["rotations"] = np.tile(F([0, 0, 0, 1]), (2, 1))      # (so that the burst is not turned away)
        chain2["clips"] = [(name, [c for c in ch if c["path"] != "rotation"]) for name, ch in chain2["clips"]] + [burst_clip()]
        self.desc["chain2"] = self.desc["spare"] = tame(chain2)
        self.desc["tree257"] = tame(make_rig("tree257", joints="all", num_targets=3, keys=(1, 2, 33)), 0.05)
        self.desc["morph"] = make_rig("chain2", joints="none", num_targets=2, keys=(2, 5))
        nodes = tame(make_rig("tree12", seed=4, joints="none", num_targets=0, keys=(2, 5)))
        nodes["clips"] = nodes["clips"] + [vanish_clip(3)]
        self.desc["crowd"] = self.desc["pair"] = nodes
        for name, d in self.desc.items():
            self.rig[name] = frt.Rig(**d, nodes_only=name in ("crowd", "pair"))
        rng = np.random.default_rng(5)
        crowd_ids = rng.permutation([i for i in range(FIRST_CHARACTER_INSTANCE) if i not in (7, TALL_BOX)])
        assert len(crowd_ids) == 300
        root = near_identity(rng, 1)[0]
        off = near_identity(rng, 300, 0.02)
        off[:, [0, 5, 10]] *= F(0.05)
        self.kw["crowd"] = {"instance_ids": crowd_ids, "nodes": rng.integers(0, 12, 300), "root": root, "offsets": off}
        self.kw["pair"] = {"instance_ids": [TALL_BOX, 7], "nodes": [3, 0]}

    def is_instances(self, name):
        return name in self.kw

    def bind_meshes(self, target, geo, names):
        """What the characters' rigs imply, bound to their meshes on `target` (a renderer or a host scene)."""
        for name in names:
            rig = self.rig[name]
            for m in self.MESHES[name]:
                n = len(geo[m].positions)
                if rig.num_targets:
                    target.set_mesh_morph_targets(m, F(0.05) * make_targets(n, rig.num_targets, seed=m))
                if rig.num_joints:
                    target.set_mesh_skin(m, *make_skin(n, rig.num_joints, seed=m), num_joints=rig.num_joints)

    def bind(self, r, geo, names):
        """{name: binding} on renderer `r`, in the order of `names`."""
        self.bind_meshes(r, geo, [n for n in names if not self.is_instances(n)])
        return {n: r.bind_rig_instances(self.rig[n], **self.kw[n]) if self.is_instances(n) else r.bind_rig(self.rig[n], self.MESHES[n]) for n in names}

    def single(self, r, b, name, clip, t):
        """The existing call for one member."""
        if self.is_instances(name):
            r.animate_instances(b[name], clip, t)
        else:
            r.animate(b[name], clip, t)

    def singles(self, r, b, rows):
        """`rows` [(name, clip, t)] through the single calls: the instance entries, then the mesh entries."""
        for want in (True, False):
            for name, clip, t in rows:
                if self.is_instances(name) == want:
                    self.single(r, b, name, clip, t)

    def host_entry(self, name, clip, t):
        """One entry of SceneBuilder.animate_cast / MultiRenderer.animate_cast."""
        if self.is_instances(name):
            return dict(rig=self.rig[name], clip=clip, t=t, **self.kw[name])
        return (self.rig[name], self.MESHES[name], clip, t)

    def times(self, name):
        return three_times(self.desc[name])
