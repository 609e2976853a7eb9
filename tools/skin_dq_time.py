"""Cost of dual-quaternion skinning beside the linear blend (include/frt.h: frt_renderer_set_mesh_skin_ex; DESIGN.md section 11, "Dual-quaternion
skinning"). Scenes: the Cornell Box's sphere (642 vertices), the 82k-triangle blob, and a character of 16 meshes (162 vertices each) under one
64-joint palette on the Cornell Box (tools/pose_batch_time.py: add_character). Rows, every call with normals="recompute" and a device palette,
microseconds per call by HIP events on the renderer's stream around the call (tools/skin_time.py: call_us), the median of 20:
  single meshes:  set_mesh_pose, the mesh bound linear / bound dual-quaternion
  the character:  set_mesh_poses over the 16 meshes, all linear / all dual-quaternion / mixed (every second mesh dual-quaternion: both skin launches)
One JSON line per scene; run it three times in fresh processes for the rounds. The dual-quaternion cost is the difference from the linear row of the
same run. With --linear-only the dual-quaternion and mixed rows are left out and no `mode` is passed: the file then runs unchanged in a checkout of
a commit that has no skin mode, for the comparison of the linear rows. Usage: python tools/skin_dq_time.py [--linear-only] [cornell blob character]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import scene_of
from mesh_update_time import mesh_of
from skin_time import synthetic_skin, call_us
from pose_batch_time import add_character

F = np.float32
NJ = 64
LINEAR_ONLY = "--linear-only" in sys.argv


def bind(r, mesh, j, w, mode):
    if LINEAR_ONLY:
        r.set_mesh_skin(mesh, j, w, num_joints=NJ)
    else:
        r.set_mesh_skin(mesh, j, w, num_joints=NJ, mode=mode)


def rigid_palettes(njoints, count=2):
    """Rotations of up to a radian times a uniform scale near 1: what the mode is for (skin_time's palettes are near the identity with shear)."""
    out = []
    for k in range(count):
        rng = np.random.default_rng(100 * njoints + k)
        m = np.zeros((njoints, 16), F)
        for j in range(njoints):
            a = rng.standard_normal(3); a /= np.linalg.norm(a)
            t = rng.uniform(-1.0, 1.0)
            K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            R = (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)) * rng.uniform(0.95, 1.05)
            M = np.eye(4); M[:3, :3] = R; M[:3, 3] = 0.01 * rng.standard_normal(3)
            m[j] = M.T.reshape(16)
        out.append(m)
    return out


def timed(r, rs, fn):
    fn(); r.sync()
    us, host = call_us(rs, rs, fn, r.sync)
    return {"us": us, "us_host": host}


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    W, H = 256, 144      # (no frame is timed here)
    for name in names:
        fs, _ = scene_of("cornell" if name == "character" else name, orc)
        r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
        dev = torch.device("cuda", r.device)
        rs = torch.cuda.ExternalStream(r.stream_handle(0))
        d_pals = [torch.from_numpy(m).to(dev) for m in rigid_palettes(NJ)]
        k = [0]
        rows = {}
        if name == "character":
            ids, geo = add_character(r, 16)
            pos = np.ascontiguousarray(geo.positions, F)
            skins = [synthetic_skin(pos, NJ, seed=m) for m in ids]
            def call():
                k[0] ^= 1; r.set_mesh_poses(ids, d_pals[k[0]])
            for row, modes in (("set_mesh_poses_linear", ["linear"] * 16), ("set_mesh_poses_dual_quaternion", ["dual_quaternion"] * 16),
                               ("set_mesh_poses_mixed", ["linear", "dual_quaternion"] * 8), ("set_mesh_poses_linear_again", ["linear"] * 16)):
                if LINEAR_ONLY and "dual_quaternion" in modes:
                    continue
                for m, s, mode in zip(ids, skins, modes):
                    r.set_mesh_vertices(m, pos); bind(r, m, *s, mode)
                rows[row] = timed(r, rs, call)
            verts = 16 * len(pos)
        else:
            mesh, geo = mesh_of(name)
            pos = np.ascontiguousarray(geo.positions, F)
            j, w = synthetic_skin(pos, NJ)
            def call():
                k[0] ^= 1; r.set_mesh_pose(mesh, d_pals[k[0]])
            for row, mode in (("set_mesh_pose_linear", "linear"), ("set_mesh_pose_dual_quaternion", "dual_quaternion"), ("set_mesh_pose_linear_again", "linear")):
                if LINEAR_ONLY and mode != "linear":
                    continue
                r.set_mesh_vertices(mesh, pos); bind(r, mesh, j, w, mode)
                rows[row] = timed(r, rs, call)
            verts = len(pos)
        print(json.dumps({"scene": name, "vertices": int(verts), "joints": NJ, "rows": rows, "deform_rejects": r.deform_rejects()}), flush=True)
        del r


if __name__ == "__main__":
    main([a for a in sys.argv[1:] if not a.startswith("--")] or ["cornell", "blob", "character"])
