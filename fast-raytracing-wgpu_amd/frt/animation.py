"""frt.Rig: a node hierarchy, a joint list and keyframed clips (include/frt.h: frt_rig_*; DESIGN.md section 11, "Animation"). The arithmetic is
libfrt.so's: evaluate() is frt_rig_evaluate, the host specification of what Renderer.animate computes on the device."""
import ctypes as C
import numpy as np
from ._lib import lib, check, FrtError, RigChannel, RigClip, RigDesc, RIG_PATHS, RIG_INTERPOLATIONS


def _f32(a, shape, what):
    a = np.ascontiguousarray(a, np.float32)
    if a.shape != shape:
        raise FrtError(f"Rig: {what} must be shaped {list(shape)}, not {list(a.shape)}")
    return a


class Rig:
    """Rig(parents, ...): nodes are given parents first (parents[n] is -1 or a smaller index).
    translations [N, 3], rotations [N, 4] (x, y, z, w), scales [N, 3]: the rest values (default: identity). matrices: {node: column-major 4x4 as [16] or
    [4, 4]} for nodes given as a matrix, which cannot be animated. joint_nodes [J] and inverse_bind [J, 16] or [J, 4, 4] (default: identities): the
    skin. num_targets and default_weights [T]: the morph targets. clips: a sequence of (name, channels), a channel a dict with node, path
    ("translation", "rotation", "scale", "weights"), interpolation ("STEP", "LINEAR", "CUBICSPLINE"), times [K] and values [K, width] (CUBICSPLINE:
    [K, 3, width] as in-tangent, value, out-tangent), width 3, 4, 3 or T by path. nodes_only=True (frt_rig_create_ex with FRT_RIG_NODES_ONLY): a
    rig with neither joints nor targets is accepted, for evaluate_nodes and Renderer.bind_rig_instances."""

    def __init__(self, parents, translations=None, rotations=None, scales=None, matrices=None, joint_nodes=(), inverse_bind=None, num_targets=0,
                 default_weights=None, clips=(), nodes_only=False):
        par = np.ascontiguousarray(parents, np.int32).reshape(-1)
        n = par.size
        trs = np.zeros((n, 10), np.float32)
        trs[:, 6] = 1.0
        trs[:, 7:10] = 1.0
        if translations is not None:
            trs[:, 0:3] = _f32(translations, (n, 3), "translations")
        if rotations is not None:
            trs[:, 3:7] = _f32(rotations, (n, 4), "rotations")
        if scales is not None:
            trs[:, 7:10] = _f32(scales, (n, 3), "scales")
        has = np.zeros(n, np.uint8)
        mats = np.zeros((n, 16), np.float32)
        for k, m in (matrices or {}).items():
            if not 0 <= int(k) < n:
                raise FrtError(f"Rig: matrices names node {k} of {n}")
            has[int(k)] = 1
            mats[int(k)] = _f32(np.asarray(m, np.float32).reshape(-1), (16,), "a node matrix")
        joints = np.ascontiguousarray(joint_nodes, np.int64).reshape(-1)
        if joints.size and (joints.min() < 0 or joints.max() > 0xFFFFFFFF):
            raise FrtError("Rig: joint nodes must be unsigned 32-bit indices")
        joints = joints.astype(np.uint32)
        ib = None if inverse_bind is None else _f32(np.asarray(inverse_bind, np.float32).reshape(-1, 16), (joints.size, 16), "inverse_bind")
        t = int(num_targets)
        dw = None if default_weights is None else _f32(default_weights, (t,), "default_weights")
        keep = [par, trs, has, mats, joints, ib, dw]      # (what the description points into, alive until frt_rig_create has copied it)
        cclips = (RigClip * max(len(clips), 1))()
        for c, (name, channels) in enumerate(clips):
            cch = (RigChannel * max(len(channels), 1))()
            for k, ch in enumerate(channels):
                if ch["path"] not in RIG_PATHS or ch.get("interpolation", "LINEAR") not in RIG_INTERPOLATIONS:
                    raise FrtError(f"Rig: clip {c}, channel {k}: unknown path or interpolation")
                path, interp = RIG_PATHS[ch["path"]], RIG_INTERPOLATIONS[ch.get("interpolation", "LINEAR")]
                times = np.ascontiguousarray(ch["times"], np.float32).reshape(-1)
                width = (3, 4, 3, t)[path]
                values = _f32(ch["values"], (times.size, 3, width) if interp == 2 else (times.size, width), f"clip {c}, channel {k}: values")
                node = int(ch.get("node", 0))
                if not 0 <= node <= 0xFFFFFFFF:
                    raise FrtError(f"Rig: clip {c}, channel {k}: node must be an unsigned 32-bit index")
                cch[k] = RigChannel(node, path, interp, times.size, times.ctypes.data, values.ctypes.data)
                keep += [times, values]
            cclips[c] = RigClip(str(name).encode(), len(channels), cch)
            keep.append(cch)
        d = RigDesc(n, par.ctypes.data, trs.ctypes.data, has.ctypes.data, mats.ctypes.data, joints.size, joints.ctypes.data if joints.size else None,
                    ib.ctypes.data if ib is not None else None, t, dw.ctypes.data if dw is not None else None, len(clips), cclips)
        h = lib().frt_rig_create_ex(C.byref(d), 1) if nodes_only else lib().frt_rig_create(C.byref(d))
        del keep
        self._adopt(h, "frt_rig_create")
        self._parents = par

    def _adopt(self, handle, call):
        self._destroy = lib().frt_rig_destroy
        self._h = handle
        if not self._h:
            raise FrtError(f"{call} failed: {lib().frt_last_error().decode()}")
        counts = (C.c_uint32 * 4)()
        check(lib().frt_rig_counts(self._h, C.byref(counts)))
        self.num_nodes, self.num_joints, self.num_targets, self.num_clips = (int(x) for x in counts)

    @classmethod
    def from_model(cls, model, skin=0):
        """The rig of skin `skin` of a loaded glTF document (frt.loader.Model; include/frt.h: frt_rig_from_model); skin=None: a morph-only rig."""
        rig = cls.__new__(cls)
        rig._adopt(lib().frt_rig_from_model(model._h, -1 if skin is None else int(skin)), "frt_rig_from_model")
        rig._parents = model.nodes()["parents"]
        return rig

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    @property
    def clips(self):
        """[(name, duration)] in clip order; the duration is the largest last key time of the clip's channels."""
        out = []
        for c in range(self.num_clips):
            name, dur = C.c_char_p(), C.c_float()
            check(lib().frt_rig_clip_info(self._h, c, C.byref(name), C.byref(dur)))
            out.append((name.value.decode(), float(dur.value)))
        return out

    def clip_index(self, clip):
        """A clip given by number or by name."""
        if isinstance(clip, str):
            names = [n for n, _ in self.clips]
            if clip not in names:
                raise FrtError(f"Rig: no clip named {clip!r} (clips: {names})")
            return names.index(clip)
        if not 0 <= int(clip) <= 0xFFFFFFFF:
            raise FrtError("Rig: a clip is a name or an unsigned 32-bit index")
        return int(clip)

    def evaluate(self, clip, t):
        """(palette [J, 16] float32 column-major or None for a rig without joints, weights [T] float32 or None for a rig without targets) of `clip` at
        time `t` (include/frt.h: frt_rig_evaluate): what set_mesh_poses takes."""
        pal = np.zeros((self.num_joints, 16), np.float32) if self.num_joints else None
        w = np.zeros(self.num_targets, np.float32) if self.num_targets else None
        check(lib().frt_rig_evaluate(self._h, self.clip_index(clip), float(t), pal.ctypes.data if pal is not None else None, w.ctypes.data if w is not None else None))
        return pal, w

    def evaluate_nodes(self, clip, t, nodes, root=None, offsets=None):
        """float32 [n, 16], column-major: (root * global[nodes[k]]) * offsets[k] of `clip` at time `t` (include/frt.h: frt_rig_evaluate_nodes), the
        matrices Renderer.animate_instances gives the instances bound to those nodes. nodes: the node numbers the rig was described with. root [16] or
        [4, 4] and offsets [n, 16] or [n, 4, 4]; None is no multiplication."""
        n, nodes, root, offsets = node_args(nodes, root, offsets)
        out = np.zeros((n, 16), np.float32)
        check(lib().frt_rig_evaluate_nodes(self._h, self.clip_index(clip), float(t), n, nodes.ctypes.data, root.ctypes.data if root is not None else None,
                                           offsets.ctypes.data if offsets is not None else None, out.ctypes.data))
        return out


    # ---- blending clips (include/frt.h: frt_rig_evaluate_blend; DESIGN.md section 11, "Blending clips")
    def sample_rows(self, samples):
        """[(clip index, t, weight)] of `samples`, an iterable of (clip, t, weight) with a clip a number or a name."""
        rows = []
        for k, s in enumerate(samples):
            s = tuple(s)
            if len(s) != 3:
                raise FrtError(f"Rig: sample {k} has {len(s)} fields, not (clip, t, weight)")
            rows.append((self.clip_index(s[0]), float(s[1]), float(s[2])))
        return rows

    def evaluate_blend(self, samples):
        """evaluate() of a blend: `samples` is [(clip, t, weight), ...], 1 to MAX_BLEND_SAMPLES of them, a clip a number or a name. Weights are
        not negative, need not sum to one, and at least one is positive. The samples are folded in order into one running pose per node: translation
        and scale mixed, the rotation slerped, each by w / (sum of the weights so far), in front of the local matrix. One sample, or every other
        weight zero, is evaluate(clip, t) bit for bit."""
        pal = np.zeros((self.num_joints, 16), np.float32) if self.num_joints else None
        w = np.zeros(self.num_targets, np.float32) if self.num_targets else None
        n, table = sample_table(self.sample_rows(samples))
        check(lib().frt_rig_evaluate_blend(self._h, n, table, pal.ctypes.data if pal is not None else None, w.ctypes.data if w is not None else None))
        return pal, w

    def evaluate_nodes_blend(self, samples, nodes, root=None, offsets=None):
        """evaluate_nodes() of a blend (`samples` as evaluate_blend takes them): the matrices Renderer.animate_instances_blend gives the instances."""
        n, nodes, root, offsets = node_args(nodes, root, offsets)
        out = np.zeros((n, 16), np.float32)
        ns, table = sample_table(self.sample_rows(samples))
        check(lib().frt_rig_evaluate_nodes_blend(self._h, ns, table, n, nodes.ctypes.data, root.ctypes.data if root is not None else None,
                                                 offsets.ctypes.data if offsets is not None else None, out.ctypes.data))
        return out

    # ---- layering clips (include/frt.h: frt_rig_evaluate_layers; DESIGN.md section 11, "Layering clips")
    def mask(self, nodes, value=1.0, descendants=True, base=0.0):
        """A mask, float32 [num_nodes] in the node order the rig was described with: `value` on `nodes` (one node or several) and, with
        descendants=True, on everything below them; `base` elsewhere. Values lie in [0, 1]."""
        m = np.full(self.num_nodes, base, np.float32)
        picked = np.zeros(self.num_nodes, bool)
        for n in np.atleast_1d(np.asarray(nodes, np.int64)):
            if not 0 <= n < self.num_nodes:
                raise FrtError(f"Rig.mask: node {n} is not a node ({self.num_nodes} nodes)")
            picked[n] = True
        if descendants:
            for n, p in enumerate(self._parents):      # (parents first: a parent's mark is final when its children are reached)
                if p >= 0 and picked[p]:
                    picked[n] = True
        m[picked] = value
        return m

    def _layer_rows(self, layers):
        """[ClipLayer] of `layers`, an iterable of frt.Layer or of plain (clip, t, weight) tuples, which are blend layers; clips by number or name."""
        from ._lib import ClipLayer, LAYER_MODES, LAYER_NO_MASK, LAYER_KEEP_MORPH
        rows = []
        for k, x in enumerate(layers):
            if not isinstance(x, Layer):
                x = tuple(x)
                if len(x) != 3:
                    raise FrtError(f"Rig: layer {k} has {len(x)} fields, not (clip, t, weight); give a frt.Layer for anything else")
                x = Layer(*x)
            if x.mode not in LAYER_MODES:
                raise FrtError(f"Rig: layer {k}: unknown mode {x.mode!r} (modes: {sorted(LAYER_MODES)})")
            if x.mask is not None and not 0 <= int(x.mask) < LAYER_NO_MASK:
                raise FrtError(f"Rig: layer {k}: a mask is None or the index of one of the masks")
            ref = x.reference
            if x.mode == "additive":
                ref = (x.clip, 0.0) if ref is None else tuple(ref)
                if len(ref) != 2:
                    raise FrtError(f"Rig: layer {k}: reference is (clip, t)")
                ref = (self.clip_index(ref[0]), float(ref[1]))
            elif ref is not None:
                raise FrtError(f"Rig: layer {k}: only an additive layer has a reference")
            else:
                ref = (0, 0.0)
            rows.append(ClipLayer(self.clip_index(x.clip), float(x.t), float(x.weight), LAYER_NO_MASK if x.mask is None else int(x.mask), LAYER_MODES[x.mode],
                                  ref[0], ref[1], 0 if x.morph else LAYER_KEEP_MORPH))
        return rows

    def _mask_args(self, masks):
        """(nmasks, float32 [nmasks, num_nodes] or None) of `masks`: None, one mask [num_nodes] or several [nmasks, num_nodes]."""
        if masks is None or len(masks) == 0:
            return 0, None
        m = np.ascontiguousarray(masks, np.float32)
        if m.ndim == 1:
            m = m[None, :]
        return m.shape[0], _f32(m, (m.shape[0], self.num_nodes), "masks")

    # ---- inverse kinematics (include/frt.h: frt_rig_evaluate_layers_ik; DESIGN.md section 11, "Inverse kinematics")
    def _goal_rows(self, goals):
        """(n, frt_rig_goal [n] or None) of `goals`: None, or an iterable of frt.TwoBone, frt.Aim and frt.Chain with the node numbers the rig was
        described with."""
        from ._lib import RigGoal, GOAL_KINDS, GOAL_CHAIN
        rows = []
        for k, g in enumerate(goals if goals is not None else ()):
            if isinstance(g, TwoBone):
                nodes, kind, axis = (g.root, g.mid, g.tip), GOAL_KINDS["two_bone"], (0.0, 0.0, 0.0)
            elif isinstance(g, Aim):
                axis = tuple(float(x) for x in g.axis)
                if len(axis) != 3:
                    raise FrtError(f"Rig: goal {k}: an axis has three components")
                nodes, kind = (g.node, 0, 0), GOAL_KINDS["aim"]
            elif isinstance(g, Chain):
                nodes, kind, axis = (g.root, g.sweeps, g.tip), GOAL_CHAIN, (0.0, 0.0, 0.0)      # (a chain's `mid` word is its number of sweeps)
            else:
                raise FrtError(f"Rig: goal {k} is neither a frt.TwoBone nor a frt.Aim nor a frt.Chain")
            if not all(0 <= int(x) <= 0xFFFFFFFF for x in nodes):
                raise FrtError(f"Rig: goal {k}: nodes (and a chain's sweeps) are unsigned 32-bit numbers")
            rows.append(RigGoal(kind, int(nodes[0]), int(nodes[1]), int(nodes[2]), (C.c_float * 3)(*axis), 0))
        return len(rows), ((RigGoal * len(rows))(*rows) if rows else None)

    def _goal_args(self, goals, targets):
        """(n, frt_rig_goal [n] or None, float32 [n, 8] or None): `targets` rows are (target xyz, weight, pole xyz, pole flag), one per goal."""
        n, table = self._goal_rows(goals)
        if targets is None:
            if n:
                raise FrtError("Rig: goals need targets, float32 [G, 8] rows of (target xyz, weight, pole xyz, pole flag)")
            return 0, None, None
        t = goal_target_rows(targets)
        if t.shape[0] != n:
            raise FrtError(f"Rig: {t.shape[0]} targets for {n} goals")
        return n, table, (t if n else None)

    def evaluate_layers(self, layers, masks=None, goals=None, targets=None):
        """evaluate() of a stack of layers (frt.Layer, or (clip, t, weight) for a blend layer), 1 to MAX_LAYERS of them, folded in order into one
        running pose per node. The first is the base: a blend layer without a mask and with a positive weight. A later layer acts by its weight
        times its mask's value at the node: "blend" mixes as evaluate_blend does, "override" replaces by that much (weight <= 1), "additive" adds
        that much of (clip at t) - (reference). masks: [nmasks, num_nodes] values in [0, 1] (Rig.mask), which Layer.mask names by index.
        goals (frt.TwoBone, frt.Aim, frt.Chain; at most MAX_RIG_GOALS) and targets ([G, 8] float32 rows of target xyz, weight, pole xyz, pole flag) act on
        the layered pose's global matrices in the rig's model space, in list order (frt_rig_evaluate_layers_ik); without goals the plain call."""
        pal = np.zeros((self.num_joints, 16), np.float32) if self.num_joints else None
        w = np.zeros(self.num_targets, np.float32) if self.num_targets else None
        n, table = layer_table(self._layer_rows(layers))
        nm, m = self._mask_args(masks)
        ng, gtable, t = self._goal_args(goals, targets)
        out = (pal.ctypes.data if pal is not None else None, w.ctypes.data if w is not None else None)
        if ng:
            check(lib().frt_rig_evaluate_layers_ik(self._h, n, table, nm, m.ctypes.data if m is not None else None, ng, gtable, t.ctypes.data, *out))
        else:
            check(lib().frt_rig_evaluate_layers(self._h, n, table, nm, m.ctypes.data if m is not None else None, *out))
        return pal, w

    def evaluate_nodes_layers(self, layers, nodes, root=None, offsets=None, masks=None, goals=None, targets=None):
        """evaluate_nodes() of a stack of layers (as evaluate_layers takes them, goals and targets included): the matrices
        Renderer.animate_instances_layers gives the instances. Goals act in the rig's model space, in front of root and offsets."""
        n, nodes, root, offsets = node_args(nodes, root, offsets)
        out = np.zeros((n, 16), np.float32)
        nl, table = layer_table(self._layer_rows(layers))
        nm, m = self._mask_args(masks)
        ng, gtable, t = self._goal_args(goals, targets)
        tail = (n, nodes.ctypes.data, root.ctypes.data if root is not None else None, offsets.ctypes.data if offsets is not None else None, out.ctypes.data)
        if ng:
            check(lib().frt_rig_evaluate_nodes_layers_ik(self._h, nl, table, nm, m.ctypes.data if m is not None else None, ng, gtable, t.ctypes.data, *tail))
        else:
            check(lib().frt_rig_evaluate_nodes_layers(self._h, nl, table, nm, m.ctypes.data if m is not None else None, *tail))
        return out


class TwoBone:
    """A two-bone goal (include/frt.h: FRT_GOAL_TWO_BONE): the limb root -> mid -> tip (mid below root, tip below mid; nodes between them are carried
    rigidly) is bent at mid so that tip's origin reaches the goal's target; its target row may carry a pole point the bend faces."""

    def __init__(self, root, mid, tip):
        self.root, self.mid, self.tip = root, mid, tip

    def __repr__(self):
        return f"TwoBone({self.root!r}, {self.mid!r}, {self.tip!r})"


class Aim:
    """An aim goal (include/frt.h: FRT_GOAL_AIM): `node` and everything below it is turned about the node's origin so that its local direction
    `axis` points at the goal's target, by the target's weight of the way."""

    def __init__(self, node, axis=(0, 0, 1)):
        self.node, self.axis = node, tuple(axis)

    def __repr__(self):
        return f"Aim({self.node!r}, axis={self.axis!r})"


class Chain:
    """A chain goal (include/frt.h: FRT_GOAL_CHAIN; DESIGN.md section 11, "Chain IK"): the parent path root -> ... -> tip (tip below root, 2 to
    IK_CHAIN_MAX_NODES nodes, every one of them a joint of the chain) is bent by `sweeps` sweeps of cyclic coordinate descent (1 to
    IK_CHAIN_MAX_SWEEPS; there is no convergence test) so that tip's origin approaches the goal's target. What hangs off a chain node moves with
    it; the tip does not turn itself. The pole words of its target row are ignored."""

    def __init__(self, root, tip, sweeps=8):
        self.root, self.tip, self.sweeps = root, tip, sweeps

    def __repr__(self):
        return f"Chain({self.root!r}, {self.tip!r}, sweeps={self.sweeps!r})"


def goal_target_rows(targets):
    """float32 [G, 8] of `targets`: rows of (target xyz, weight, pole xyz, pole flag)."""
    t = np.ascontiguousarray(targets, np.float32)
    if t.size == 0:
        t = t.reshape(0, 8)
    if t.ndim == 1 and t.size == 8:
        t = t[None, :]
    if t.ndim != 2 or t.shape[1] != 8:
        raise FrtError(f"goal targets must be shaped [G, 8] (target xyz, weight, pole xyz, pole flag), not {list(t.shape)}")
    return t


class Layer:
    """One layer of a stack (include/frt.h: frt_clip_layer): `clip` (a number or a name) at time `t`, acting by `weight` times the value of mask
    number `mask` (None: 1 everywhere) at each node. mode: "blend", "override" or "additive"; reference: (clip, t) an additive layer is the
    difference from, by default the same clip at time 0. morph=False: the layer leaves the morph weights alone."""

    def __init__(self, clip, t, weight=1.0, mask=None, mode="blend", reference=None, morph=True):
        self.clip, self.t, self.weight, self.mask, self.mode, self.reference, self.morph = clip, t, weight, mask, mode, reference, morph

    def __repr__(self):
        return f"Layer({self.clip!r}, {self.t!r}, weight={self.weight!r}, mask={self.mask!r}, mode={self.mode!r}, reference={self.reference!r}, morph={self.morph!r})"


def layer_table(rows):
    """(n, frt_clip_layer [n]) of [ClipLayer]."""
    from ._lib import ClipLayer
    return len(rows), (ClipLayer * max(len(rows), 1))(*rows)


def sample_table(rows):
    """(n, frt_clip_sample [n]) of [(clip index, t, weight)]."""
    from ._lib import ClipSample
    return len(rows), (ClipSample * max(len(rows), 1))(*[ClipSample(c, t, w, 0) for c, t, w in rows])


def node_args(nodes, root, offsets):
    """(n, nodes uint32 [n], root float32 [16] or None, offsets float32 [n, 16] or None) as the C calls of node animation take them."""
    nodes = np.ascontiguousarray(nodes, np.int64).reshape(-1)
    if nodes.size and (nodes.min() < 0 or nodes.max() > 0xFFFFFFFF):
        raise FrtError("Rig: nodes must be unsigned 32-bit indices")
    nodes = nodes.astype(np.uint32)
    if root is not None:
        root = _f32(np.asarray(root, np.float32).reshape(-1), (16,), "root")
    if offsets is not None:
        offsets = _f32(np.asarray(offsets, np.float32).reshape(-1, 16), (nodes.size, 16), "offsets")
    return nodes.size, nodes, root, offsets


def host_cast(target, entries, normals="recompute"):
    """What SceneBuilder.animate_cast and MultiRenderer.animate_cast do ("Animating a cast"): every entry is the arguments of
    `target`'s animate, (rig, mesh_ids, clip, t), or of its animate_instances, (rig, instance_ids, nodes, clip, t[, root[, offsets]]), as a tuple
    or as a dict by name (a dict with "nodes" is an instance entry). The instance entries are applied first, in the order given, then the mesh
    entries: the order of the device call's two halves."""
    inst, mesh = [], []
    for k, e in enumerate(entries):
        if isinstance(e, dict):
            (inst if "nodes" in e else mesh).append(dict(e))
            continue
        e = tuple(e)
        if len(e) == 4:
            mesh.append(dict(zip(("rig", "mesh_ids", "clip", "t"), e)))
        elif 5 <= len(e) <= 7:
            inst.append(dict(zip(("rig", "instance_ids", "nodes", "clip", "t", "root", "offsets"), e)))
        else:
            raise FrtError(f"animate_cast: entry {k} has {len(e)} fields (4: a mesh entry, 5 to 7: an instance entry)")
    if not inst and not mesh:
        raise FrtError("animate_cast: no entries")
    for e in inst:
        target.animate_instances(**e)
    for e in mesh:
        target.animate(**e, normals=normals)


def host_cast_blend(target, entries, normals="recompute"):
    """host_cast for blends ("Blending clips"): what SceneBuilder.animate_cast_blend and MultiRenderer.animate_cast_blend do.
    Every entry is the arguments of `target`'s animate_blend, (rig, mesh_ids, samples), or of its animate_instances_blend,
    (rig, instance_ids, nodes, samples[, root[, offsets]]), as a tuple or as a dict by name (a dict with "nodes" is an instance entry). The
    instance entries are applied first, in the order given, then the mesh entries."""
    inst, mesh = [], []
    for k, e in enumerate(entries):
        if isinstance(e, dict):
            (inst if "nodes" in e else mesh).append(dict(e))
            continue
        e = tuple(e)
        if len(e) == 3:
            mesh.append(dict(zip(("rig", "mesh_ids", "samples"), e)))
        elif 4 <= len(e) <= 6:
            inst.append(dict(zip(("rig", "instance_ids", "nodes", "samples", "root", "offsets"), e)))
        else:
            raise FrtError(f"animate_cast_blend: entry {k} has {len(e)} fields (3: a mesh entry, 4 to 6: an instance entry)")
    if not inst and not mesh:
        raise FrtError("animate_cast_blend: no entries")
    for e in inst:
        target.animate_instances_blend(**e)
    for e in mesh:
        target.animate_blend(**e, normals=normals)


def _is_index_list(x):
    """Whether `x` is a non-empty sequence or array of plain integers (node numbers), which no list of layers is."""
    try:
        return len(x) > 0 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in x)
    except TypeError:
        return False


def host_cast_layers(target, entries, normals="recompute"):
    """host_cast for layers ("Layering clips"): what SceneBuilder.animate_cast_layers and MultiRenderer.animate_cast_layers do.
    Every entry is the arguments of `target`'s animate_layers, (rig, mesh_ids, layers[, masks]), or of its animate_instances_layers,
    (rig, instance_ids, nodes, layers, masks[, root[, offsets]]) with masks possibly None, as a tuple or as a dict by name (a dict with "nodes" is
    an instance entry). The instance entries are applied first, in the order given, then the mesh entries. Goals ("Inverse kinematics"): a dict
    entry of either kind may carry "goals" and "targets"; an instance tuple takes them as its eighth and ninth field."""
    inst, mesh = [], []
    for k, e in enumerate(entries):
        if isinstance(e, dict):
            (inst if "nodes" in e else mesh).append(dict(e))
            continue
        e = tuple(e)
        if 3 <= len(e) <= 4:
            if len(e) == 4 and _is_index_list(e[2]):      # (rig, instance_ids, nodes, layers): an instance entry without its masks slot
                raise FrtError(f"animate_cast_layers: entry {k} has four fields and the third is a list of node numbers, not of layers: an instance "
                               "entry is (rig, instance_ids, nodes, layers, masks[, root[, offsets]]), with masks None when it has none")
            mesh.append(dict(zip(("rig", "mesh_ids", "layers", "masks"), e)))
        elif 5 <= len(e) <= 9:
            inst.append(dict(zip(("rig", "instance_ids", "nodes", "layers", "masks", "root", "offsets", "goals", "targets"), e)))
        else:
            raise FrtError(f"animate_cast_layers: entry {k} has {len(e)} fields (3 or 4: a mesh entry, 5 to 9: an instance entry)")
    if not inst and not mesh:
        raise FrtError("animate_cast_layers: no entries")
    for e in inst:
        target.animate_instances_layers(**e)
    for e in mesh:
        target.animate_layers(**e, normals=normals)
