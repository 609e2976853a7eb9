// frt_ik.hpp — the arithmetic of inverse kinematics on a rig (include/frt.h: frt_rig_evaluate_layers_ik, frt_renderer_set_rig_goals; DESIGN.md §11,
// "Inverse kinematics"). Included by frt_animation.hpp behind its own functions; every function here is FRT_HD and is the one text the host form
// (frt_animation.cpp: apply_goals) and the kernels (frt_animation.hip: rig_apply_goals) both run under the library's contract flags: f32, no
// contraction, no hand-written fma, every product and sum written once, rsqrt_exact / sqrtf_ / rcpf_ of frt_math.hpp and rig_slerp / rig_trs_matrix
// of frt_animation.hpp. No acos is taken: a rotation between two directions is built from their cross and dot products. The third kind, a CCD
// chain ("Chain IK"), is at the end of the file: it is built from ik_arc, ik_about and ik_point alone.
//
// A GOAL acts on the GLOBAL matrices of a rig, in the rig's model space, behind the hierarchy walk: it is a rotation about a pivot (an m4 `D`) that
// every node of a subtree takes as G = mul(D, G). Nodes are stored by depth, so a subtree is not a range of the block: `enter` / `exit` are pre-order
// numbers per stored node (frt_animation.cpp: rig_tree), and d lies in subtree(a) iff enter[a] <= enter[d] < exit[a].
#pragma once

namespace frt {

FRT_HD bool ik_finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }
// Step 1 of both kinds: a target record takes part when its eight words are finite and its weight lies in (0, 1]. The host calls refuse what this
// skips (but a weight of 0); a record in device memory is seen here first.
FRT_HD bool ik_target_ok(const frt_rig_goal_target& t) {
    const bool fin = ik_finite(t.target[0]) && ik_finite(t.target[1]) && ik_finite(t.target[2]) && ik_finite(t.weight) &&
                     ik_finite(t.pole[0]) && ik_finite(t.pole[1]) && ik_finite(t.pole[2]) && ik_finite(t.pole_flag);
    return fin && t.weight > 0.0f && t.weight <= 1.0f;
}
// The shortest-arc rotation that takes the unit vector u to the unit vector v: (cross(u, v), 1 + dot(u, v)) normalised. Antiparallel vectors
// (1 + dot below FRT_IK_ARC_EPS) have no shortest arc: a half turn about cross(u, e), e the coordinate axis of u's smallest |component| (the first
// of equals).
FRT_HD f4 ik_arc(f3 u, f3 v) {
    const float d = 1.0f + dot(u, v);
    if (d < FRT_IK_ARC_EPS) {
        const float ax = fabsf_(u.x), ay = fabsf_(u.y), az = fabsf_(u.z);
        const f3 e = (ax <= ay && ax <= az) ? mk3(1.0f, 0.0f, 0.0f) : (ay <= az ? mk3(0.0f, 1.0f, 0.0f) : mk3(0.0f, 0.0f, 1.0f));
        return mk4(normalize(cross(u, e)), 0.0f);
    }
    const f4 q = mk4(cross(u, v), d);
    return q * rsqrt_exact(rig_dot4(q, q));
}
// The rotation q about the point p: the 3x3 of rig_trs_matrix (its nine products; a scale of one changes no bit), the last column p - R p.
FRT_HD m4 ik_about(f3 p, f4 q) {
    m4 m = rig_trs_matrix(mk3(0.0f, 0.0f, 0.0f), q, mk3(1.0f, 1.0f, 1.0f));
    const f3 rp = (xyz(m.c[0]) * p.x + xyz(m.c[1]) * p.y) + xyz(m.c[2]) * p.z;
    m.c[3] = mk4(p - rp, 1.0f);
    return m;
}
FRT_HD f3 ik_point(const m4& m, f3 p) { return xyz(mul(m, mk4(p, 1.0f))); }

// What a goal does to the globals: nothing (`on` false: the goal is skipped and nothing is written), or `inner` for every node of subtree(inner_node)
// and `outer` for every other node of subtree(outer_node). An AIM has one subtree: inner_node == outer_node and both matrices are the same.
struct IkDelta { bool on; uint32_t outer_node, inner_node; m4 outer, inner; };

// TWO_BONE: A, B, C the origins of root, mid and tip. The steps are those of include/frt.h, in that order.
FRT_HD bool ik_two_bone(f3 A, f3 B, f3 C, const frt_rig_goal_target& t, m4& da, m4& dba) {
    const f3 T = mk3(t.target[0], t.target[1], t.target[2]);
    const float w = t.weight;
    const f3 Te = w == 1.0f ? T : C + w * (T - C);
    const f3 ab = B - A, cb = C - B, at = Te - A;
    const float lab = sqrtf_(dot(ab, ab)), lcb = sqrtf_(dot(cb, cb)), d = sqrtf_(dot(at, at));
    if (!(lab > 0.0f && lcb > 0.0f && d > 0.0f)) return false;
    const f3 dir = at * rcpf_(d);
    const float lat = fminn(fmaxn(d, fabsf_(lab - lcb)), lab + lcb);
    const bool pole = t.pole_flag != 0.0f;
    f3 side = pole ? mk3(t.pole[0], t.pole[1], t.pole[2]) - A : ab;
    f3 nrm = cross(dir, side);
    if (!(dot(nrm, nrm) > FRT_IK_PLANE_EPS * dot(side, side))) {
        if (!pole) return false;
        side = ab;
        nrm = cross(dir, side);
        if (!(dot(nrm, nrm) > FRT_IK_PLANE_EPS * dot(side, side))) return false;      // a straight limb without a usable pole has no bend plane
    }
    const f3 perp = cross(normalize(nrm), dir);
    const float inv = rcpf_((2.0f * lab) * lat);
    const float c = clampf(((lab * lab + lat * lat) - lcb * lcb) * inv, -1.0f, 1.0f);
    // s, the sine of the angle at A, from the triangle's area (Heron's product) and not from sqrt(1 - c c): at full stretch or fully folded c is 1 to
    // rounding and 1 - c c would turn c's last bit into 5e-4 of a bone length across the limb. Each factor is a difference of the lengths themselves:
    // a clamped lat (lab + lcb, or |lab - lcb|) makes one of them exactly 0, and s with it.
    const float h = fmaxn((((lat + (lcb - lab)) * ((lab + lcb) - lat)) * (lat + (lab - lcb))) * ((lab + lcb) + lat), 0.0f);
    const float s = sqrtf_(h) * inv;
    const f3 B1 = A + lab * (c * dir + s * perp);
    const f3 C2 = A + lat * dir;
    da = ik_about(A, ik_arc(normalize(ab), normalize(B1 - A)));
    const f3 C1 = ik_point(da, C);
    const m4 db = ik_about(B1, ik_arc(normalize(C1 - B1), normalize(C2 - B1)));
    dba = mul(db, da);
    return true;
}
// AIM: the local direction `axis` of the node whose global is G is turned towards the target, by the weight's share of the arc.
FRT_HD bool ik_aim(const m4& G, f3 axis, const frt_rig_goal_target& t, m4& d) {
    const f3 O = xyz(G.c[3]);
    const f3 v = (xyz(G.c[0]) * axis.x + xyz(G.c[1]) * axis.y) + xyz(G.c[2]) * axis.z;
    const f3 to = mk3(t.target[0], t.target[1], t.target[2]) - O;
    if (!(sqrtf_(dot(v, v)) > 0.0f && sqrtf_(dot(to, to)) > 0.0f)) return false;
    f4 q = ik_arc(normalize(v), normalize(to));
    if (t.weight < 1.0f) q = rig_slerp(mk4(0.0f, 0.0f, 0.0f, 1.0f), q, t.weight);
    d = ik_about(O, q);
    return true;
}
// One goal (stored node indices) under its target, given the globals of its root, mid and tip as the earlier goals left them (an AIM reads the
// first only).
FRT_HD IkDelta ik_goal_delta(const frt_rig_goal& g, const frt_rig_goal_target& t, const m4& Groot, const m4& Gmid, const m4& Gtip) {
    IkDelta r;
    r.on = false; r.outer_node = g.root; r.inner_node = g.root;
    if (!ik_target_ok(t)) return r;
    if (g.kind == (uint32_t)FRT_GOAL_AIM) {
        r.on = ik_aim(Groot, mk3(g.axis[0], g.axis[1], g.axis[2]), t, r.outer);
        r.inner = r.outer;
        return r;
    }
    r.inner_node = g.mid;
    r.on = ik_two_bone(xyz(Groot.c[3]), xyz(Gmid.c[3]), xyz(Gtip.c[3]), t, r.outer, r.inner);
    return r;
}
FRT_HD bool ik_in_subtree(const uint32_t* enter, const uint32_t* exit, uint32_t a, uint32_t n) { return enter[a] <= enter[n] && enter[n] < exit[a]; }
// Node n under a goal that is on: false when it keeps its global, else G = mul(D, G) with the matrix of the subtree it lies in.
FRT_HD bool ik_move_node(const IkDelta& d, const uint32_t* enter, const uint32_t* exit, uint32_t n, m4& G) {
    if (ik_in_subtree(enter, exit, d.inner_node, n)) { G = mul(d.inner, G); return true; }
    if (ik_in_subtree(enter, exit, d.outer_node, n)) { G = mul(d.outer, G); return true; }
    return false;
}

// CHAIN ("Chain IK"): cyclic coordinate descent over the parent path c_0 = root .. c_K = tip. P_j the origin of G[c_j] and D_j the identity at the
// start; the caller (frt_animation.cpp: apply_chain_goal over arrays; frt_animation.hip: rig_apply_chain over the lanes of a wave) runs S sweeps of
// k = K - 1 .. 0 and, where ik_chain_step says so, takes P_j = ik_point(R, P_j) for j > k and D_j = mul(R, D_j) for j >= k. These two functions
// are all the arithmetic and all the decisions of a sweep: both callers only index.
FRT_HD f3 ik_chain_target(f3 tip, const frt_rig_goal_target& t) {
    const f3 T = mk3(t.target[0], t.target[1], t.target[2]);
    const float w = t.weight;
    return w == 1.0f ? T : tip + w * (T - tip);
}
// One step at joint k: the rotation about Pk that turns the tip PK towards Te; false (the step changes nothing) when either length is not > 0.
FRT_HD bool ik_chain_step(f3 Pk, f3 PK, f3 Te, m4& R) {
    const f3 e = PK - Pk, t = Te - Pk;
    if (!(sqrtf_(dot(e, e)) > 0.0f && sqrtf_(dot(t, t)) > 0.0f)) return false;
    R = ik_about(Pk, ik_arc(normalize(e), normalize(t)));
    return true;
}
FRT_HD m4 ik_identity() {
    m4 m;
    m.c[0] = mk4(1.0f, 0.0f, 0.0f, 0.0f); m.c[1] = mk4(0.0f, 1.0f, 0.0f, 0.0f); m.c[2] = mk4(0.0f, 0.0f, 1.0f, 0.0f); m.c[3] = mk4(0.0f, 0.0f, 0.0f, 1.0f);
    return m;
}

} // namespace frt
