"""Small rigged glTF / GLB documents for the loader's rig tests (tests/test_loader_rig.py, tests/test_animation_gpu.py): one base64 (or BIN chunk)
buffer, accessors appended as they are asked for, and the character the tests load, with the arrays it was written from."""
import base64
import json
import struct
import numpy as np

F = np.float32
COMP = {np.dtype(np.int8): 5120, np.dtype(np.uint8): 5121, np.dtype(np.int16): 5122, np.dtype(np.uint16): 5123, np.dtype(np.uint32): 5125, np.dtype(np.float32): 5126}
TYPE = {1: "SCALAR", 2: "VEC2", 3: "VEC3", 4: "VEC4", 16: "MAT4"}


class RigWriter:
    def __init__(self):
        self.bin = bytearray()
        self.doc = {"asset": {"version": "2.0"}, "buffers": [{}], "bufferViews": [], "accessors": [], "meshes": [], "nodes": [], "skins": [], "animations": []}

    def accessor(self, arr, normalized=False, count=None):
        a = np.ascontiguousarray(arr)
        a = a.reshape(len(a), -1)
        while len(self.bin) % 4:
            self.bin.append(0)
        self.doc["bufferViews"].append({"buffer": 0, "byteOffset": len(self.bin), "byteLength": a.nbytes})
        self.bin += a.tobytes()
        acc = {"bufferView": len(self.doc["bufferViews"]) - 1, "componentType": COMP[a.dtype], "count": len(a) if count is None else count, "type": TYPE[a.shape[1]]}
        if normalized:
            acc["normalized"] = True
        self.doc["accessors"].append(acc)
        return len(self.doc["accessors"]) - 1

    def sampler(self, anim, times, values, interpolation):
        anim.setdefault("samplers", []).append({"input": self.accessor(np.asarray(times, F)), "output": values, "interpolation": interpolation})
        return len(anim["samplers"]) - 1

    def json(self, uri=True):
        d = {k: v for k, v in self.doc.items() if v or k in ("asset", "buffers")}
        d["buffers"] = [{"byteLength": len(self.bin)}]
        if uri:
            d["buffers"][0]["uri"] = "data:application/octet-stream;base64," + base64.b64encode(bytes(self.bin)).decode()
        return json.dumps(d)

    def save_gltf(self, path):
        open(path, "w").write(self.json())

    def save_glb(self, path):
        js = self.json(uri=False).encode()
        js += b" " * (-len(js) % 4)
        body = bytes(self.bin) + b"\0" * (-len(self.bin) % 4)
        out = struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(body), 0x004E4942) + body
        open(path, "wb").write(struct.pack("<III", 0x46546C67, 2, 12 + len(out)) + out)


def unit(q):
    q = np.asarray(q, np.float64)
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(F)


def character(seed=0):
    """(writer, ref): one mesh of two primitives (4 and 3 vertices; u8 joints with normalized-u16 weights, u16 joints with float weights; 2 targets
    each, default weights 0.25, 0.5) on node 0 under skin 0; five joints, documents nodes 3 (the root: children 1 and 4), 1 (child 2), 2, 4 (given as a
    matrix, child 5) and 5 — not parents first; skin 1 is the same joints without inverseBindMatrices; two animations with all three interpolations and
    all four paths, one rotation output as normalized int16. ref: the arrays as the loader has to return them (stored order: 0, 3, 1, 4, 2, 5)."""
    rng = np.random.default_rng(seed)
    w = RigWriter()
    ref = {"order": [0, 3, 1, 4, 2, 5]}
    pos = [rng.uniform(-0.3, 0.3, (4, 3)).astype(F), rng.uniform(-0.3, 0.3, (3, 3)).astype(F)]
    idx = [np.array([0, 1, 2, 1, 3, 2], np.uint16), np.array([0, 1, 2], np.uint16)]
    joints = [rng.integers(0, 5, (4, 4)).astype(np.uint8), rng.integers(0, 5, (3, 4)).astype(np.uint16)]
    w16 = rng.integers(0, 65536, (4, 4)).astype(np.uint16)
    wf = rng.random((3, 4)).astype(F)
    wf = (wf / wf.sum(axis=1, keepdims=True)).astype(F)
    deltas = [(0.05 * rng.standard_normal((2, 4, 3))).astype(F), (0.05 * rng.standard_normal((2, 3, 3))).astype(F)]
    prims = []
    for k in range(2):
        attrs = {"POSITION": w.accessor(pos[k]), "JOINTS_0": w.accessor(joints[k]), "WEIGHTS_0": w.accessor(w16, normalized=True) if k == 0 else w.accessor(wf)}
        prims.append({"attributes": attrs, "indices": w.accessor(idx[k]), "targets": [{"POSITION": w.accessor(deltas[k][t])} for t in range(2)]})
    w.doc["meshes"].append({"primitives": prims, "weights": [0.25, 0.5]})
    ref.update(pos=pos, idx=idx, joints=[j.astype(np.uint16) for j in joints], weights=[w16.astype(F) / F(65535.0), wf], deltas=deltas, default_weights=F([0.25, 0.5]))
    tr = (0.2 * rng.standard_normal((6, 3))).astype(F)
    ro = unit(rng.standard_normal((6, 4)))
    sc = rng.uniform(0.8, 1.25, (6, 3)).astype(F)
    mat = np.eye(4, dtype=F)
    mat[:3, :3] += (0.1 * rng.standard_normal((3, 3))).astype(F)
    mat[3, :3] = (0.1, -0.2, 0.3)
    w.doc["nodes"] = [{"mesh": 0, "skin": 0},
                      {"children": [2], "translation": tr[1].tolist()},
                      {"rotation": ro[2].tolist()},
                      {"children": [1, 4], "translation": tr[3].tolist(), "scale": sc[3].tolist()},
                      {"children": [5], "matrix": mat.reshape(16).tolist()},
                      {"rotation": ro[5].tolist(), "translation": tr[5].tolist()}]
    given = {1: ("t",), 2: ("r",), 3: ("t", "s"), 5: ("r", "t")}
    order = ref["order"]
    ref["parents"] = np.array([-1, -1, 1, 1, 2, 3], np.int32)
    ref["translations"] = np.stack([tr[d] if "t" in given.get(d, ()) else np.zeros(3, F) for d in order])
    ref["rotations"] = np.stack([ro[d] if "r" in given.get(d, ()) else F([0, 0, 0, 1]) for d in order])
    ref["scales"] = np.stack([sc[d] if "s" in given.get(d, ()) else np.ones(3, F) for d in order])
    ref["has_matrix"] = np.array([d == 4 for d in order])
    ref["matrix"] = mat.reshape(16)
    stored = {d: i for i, d in enumerate(order)}
    ibm = np.tile(np.eye(4, dtype=F).reshape(16), (5, 1))
    ibm[:, 12:15] = (0.1 * rng.standard_normal((5, 3))).astype(F)
    w.doc["skins"] = [{"joints": [3, 1, 2, 4, 5], "inverseBindMatrices": w.accessor(ibm)}, {"joints": [3, 1, 2, 4, 5]}]
    ref["skin_joints"] = np.array([stored[d] for d in (3, 1, 2, 4, 5)], np.uint32)
    ref["inverse_bind"] = ibm
    # animations
    t3, t2 = F([0.0, 0.5, 1.25]), F([0.25, 1.0])
    a_tr = (0.2 * rng.standard_normal((3, 3))).astype(F)
    a_ro = rng.standard_normal((3, 3, 4)).astype(F)
    a_ro[:, 1] = unit(a_ro[:, 1])
    a_w = rng.random((2, 2)).astype(F)
    b_sc = rng.uniform(0.8, 1.25, (2, 3)).astype(F)
    q16 = np.round(unit(rng.standard_normal((3, 4))).astype(np.float64) * 32767).astype(np.int16)
    q16[0, 0] = -32768      # glTF: max(x / 32767, -1)
    a, b = {"name": "wave", "channels": []}, {"name": "nod", "channels": []}
    a["channels"] = [{"sampler": w.sampler(a, t3, w.accessor(a_tr), "LINEAR"), "target": {"node": 1, "path": "translation"}},
                     {"sampler": w.sampler(a, t3, w.accessor(a_ro.reshape(9, 4)), "CUBICSPLINE"), "target": {"node": 2, "path": "rotation"}},
                     {"sampler": w.sampler(a, t2, w.accessor(a_w.reshape(4, 1)), "STEP"), "target": {"node": 0, "path": "weights"}}]
    b["channels"] = [{"sampler": w.sampler(b, t2, w.accessor(b_sc), "STEP"), "target": {"node": 3, "path": "scale"}},
                     {"sampler": w.sampler(b, t3, w.accessor(q16, normalized=True), "LINEAR"), "target": {"node": 5, "path": "rotation"}}]
    w.doc["animations"] = [a, b]
    ref["animations"] = [("wave", [dict(node=stored[1], path="translation", interpolation="LINEAR", times=t3, values=a_tr),
                                   dict(node=stored[2], path="rotation", interpolation="CUBICSPLINE", times=t3, values=a_ro),
                                   dict(node=stored[0], path="weights", interpolation="STEP", times=t2, values=a_w)]),
                         ("nod", [dict(node=stored[3], path="scale", interpolation="STEP", times=t2, values=b_sc),
                                  dict(node=stored[5], path="rotation", interpolation="LINEAR", times=t3, values=np.maximum(q16.astype(F) / F(32767.0), F(-1.0)))])]
    return w, ref
