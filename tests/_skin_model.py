"""What the skinning tests share (include/frt.h: frt_scene_set_mesh_skin, frt_scene_set_mesh_pose; DESIGN.md section 11, "Skinning"): the float32 numpy
model of the contract, written as elementwise * and + in the stated order, and deterministic synthetic skins and palettes."""
import numpy as np

F = np.float32
JOINT_COUNTS = (1, 3, 70)


def skin_model(positions, joints, weights, mats):
    """out[r] = ((w0 q_0[r] + w1 q_1[r]) + w2 q_2[r]) + w3 q_3[r] with q_k[r] = ((M[r] x + M[4 + r] y) + M[8 + r] z) + M[12 + r] of joint j_k; out.w = p.w."""
    p = np.ascontiguousarray(positions, F)
    m = np.ascontiguousarray(mats, F).reshape(-1, 16)
    j, w = np.asarray(joints), np.ascontiguousarray(weights, F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = p.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            q = []
            for k in range(4):
                mk = m[j[:, k]]
                q.append(((mk[:, r] * x + mk[:, 4 + r] * y) + mk[:, 8 + r] * z) + mk[:, 12 + r])
            out[:, r] = ((w[:, 0] * q[0] + w[:, 1] * q[1]) + w[:, 2] * q[2]) + w[:, 3] * q[3]
    assert out.dtype == F
    return out


def plain_transform(positions, mat):
    """world_triangle's point under one matrix: what a 1-joint palette with weights (1, 0, 0, 0) must give."""
    p, m = np.ascontiguousarray(positions, F), np.ascontiguousarray(mat, F).reshape(16)
    out = p.copy()
    for r in range(3):
        out[:, r] = ((m[r] * p[:, 0] + m[4 + r] * p[:, 1]) + m[8 + r] * p[:, 2]) + m[12 + r]
    return out


def make_skin(n, njoints, seed=0):
    """(joints [n, 4] uint16, weights [n, 4] float32) for a mesh of n >= 4 vertices. Vertex 0 names joint njoints - 1; vertex 1 names one joint in all
    four slots; vertex 2 has two weights that are exactly 0 and every fifth vertex one; the weights of vertex 3 sum to 1.2; the other rows sum to 1 up to
    rounding."""
    rng = np.random.default_rng(1000 * njoints + n + seed)
    j = rng.integers(0, njoints, size=(n, 4)).astype(np.uint16)
    w = rng.random((n, 4)).astype(F) + F(0.05)
    w[::5, 3] = 0.0
    w = (w / w.sum(axis=1, keepdims=True)).astype(F)
    j[0, 0] = njoints - 1
    j[1, :] = j[1, 0]
    w[2] = (0.5, 0.0, 0.5, 0.0)
    w[3] = (0.3, 0.3, 0.3, 0.3)
    return j, w


def make_palette(njoints, phase=0.0):
    """[njoints, 16] column-major matrices near the identity (the posed mesh stays about where it was). Joint 0 mirrors x (a negative determinant);
    row 3, which the contract ignores, holds other numbers than (0, 0, 0, 1) in the last joint."""
    rng = np.random.default_rng(7 * njoints + int(round(100 * phase)))
    m = np.zeros((njoints, 4, 4), F)      # m[j, c, r]
    for k in range(njoints):
        a = np.eye(3) + 0.12 * rng.standard_normal((3, 3))
        if k == 0:
            a[:, 0] = -a[:, 0]
            assert np.linalg.det(a) < 0
        m[k, :3, :3] = a.T.astype(F) if k % 2 else a.astype(F)
        m[k, 3, :3] = (0.05 * rng.standard_normal(3)).astype(F)
        m[k, 3, 3] = 1.0
    m[njoints - 1, :, 3] = (0.25, -3.0, 7.0, 0.5)
    assert np.linalg.det(m[0, :3, :3].astype(np.float64)) < 0
    return np.ascontiguousarray(m.reshape(njoints, 16))


def overflowing_palette(njoints):
    """Finite matrices under which a skinned coordinate of any mesh with a vertex off the origin overflows to infinity."""
    m = make_palette(njoints)
    m[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]] = F(3.0e38)      # 3e38 (x + y + z) + 3e38: past the largest float for x + y + z > 0.14
    return m


def scene_with_a_spare_mesh(frt):
    """(scene, meshes, grey): a floor, a quad light, one instance of mesh 2 (a 162-vertex sphere) and one of mesh 3 (a 42-vertex sphere); mesh 1 (the
    crystal) is in the pools and unused, so remove_meshes(1) renumbers 2 and 3."""
    from frt.scenes import _T, _S, _RX, _mul
    g = frt.geometry
    meshes = [g.create_plane(), g.create_crystal(), g.create_sphere(2), g.create_sphere(1)]
    b = frt.SceneBuilder()
    for m in meshes:
        b.add_mesh(m)
    grey = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(0, grey, _mul(_T(0.0, -1.0, 0.0), _S(4.0)))
    b.register_quad_light(0, _mul(_T(0.0, 1.5, 0.0), _RX(np.pi), _S(0.5)), (1.0, 1.0, 1.0), 10.0)
    b.add_instance(2, grey, _mul(_T(-0.5, -0.4, 0.0), _S(0.6)))
    b.add_instance(3, grey, _mul(_T(0.5, -0.4, 0.1), np.diag(np.array([-0.5, 0.5, 0.5, 1.0], F))))
    return b.build(), meshes, grey
