"""A shadow model of the scene state that rt_scene_update applies: plain Python and numpy, written from DESIGN.md section 2 ("update == build",
for rigid transforms, meshes that change shape, skinned vertices and masks) and the comments of include/dxr_amd.h -- not from the library, and
with no import from it.  tests/scene_edit_sweep.py issues every operation to the GPU library and to this model and holds the two to each other:
the return code of every call, and at every successful update or build the whole scene against a fresh build of the state kept here.

The rules (numbered as the sweep's log and DESIGN.md section 6 name them):
 1. Setters on a scene that has not been built since its last add_model only store; update is refused (ERR_STATE); build brings the scene back.
 2. On an updatable scene a transform setter with count > 0 makes the scene stale.
 3. A mask setter makes the scene stale only if some instance flips between zero and non-zero; otherwise it stays fresh and masks() returns
    the new bytes.
 4. set_vertices, set_positions (count > 0), recompute_normals and set_bones make every built scene that holds the model stale.
 5. set_skin and clear_skin change no vertex and leave no scene stale.
 6. A setter with count == 0 is a no-op and returns OK.
 7. An out-of-range setter returns ERR_STATE.
 8. set_bones without a skin returns ERR_STATE.
 9. A refused skin returns ERR_INVALID_ARG and keeps the old skin.
10. After any refusal the state is what it was.
11. update with nothing pending returns OK and changes nothing (a pipeline that has rendered still answers count_work()); after a real update
    count_work() is refused until the next render.
12. update or build with every mask zero is refused (ERR_STATE) and keeps everything pending; after one instance is shown the next update
    applies all of it.
13. While a scene is stale, trace, the bvh / wide_read / refs readers and render return ERR_STATE.
14. The rest pose is the vertices at the time of set_skin.
15. set_vertices / set_positions after set_skin change the current vertices, not the rest pose; the next set_bones overwrites every vertex
    from the rest pose.
16. geometry() always returns the current vertices.
Morph targets and posed skeletons (include/dxr_amd.h "Morph targets", "Posed skeletons").  A model has up to three hidden vertex arrays next to
its current vertices -- the skin's rest pose, the morph base -- and no reader returns them: a wrong one shows through the next producer.
17. set_morph_targets changes no vertex and leaves no scene stale.  It captures the BASE: the skin's rest pose if the model has a skin then,
    otherwise the current vertices.  Calling it again replaces the targets and captures the base anew.
18. A refused set_morph_targets returns ERR_INVALID_ARG and keeps the old targets and the old base: target_offsets[0] != 0, offsets that
    decrease, a vertex index >= V, indices within a target that do not ascend strictly, more than 65536 targets.
19. clear_morph_targets removes the targets; the vertices and the rest pose stay.
20. set_morph_weights without targets returns ERR_STATE.
21. set_morph_weights on a model without a skin: the vertices = morphed(base, ...), the whole mesh, always from the base; every built scene
    that holds the model goes stale (as rule 4).
22. set_morph_weights on a model with a skin: the REST POSE = morphed(base, ...); the vertices are untouched and no scene goes stale; the next
    set_bones poses the morphed rest pose.
23. set_skin captures its rest pose from the current vertices (rule 14) and never touches the morph base; it redirects later morph results
    to the new rest pose.  clear_skin redirects them to the vertices.  Neither recaptures the base.
24. set_vertices / set_positions / recompute_normals on a morphed model write the current vertices and leave the base alone.
25. A skeleton holds parents, inverse binds, a pose, clips, and -- once posed -- world matrices and a palette.  set_pose, add_clip, clear_clips
    and set_time touch no model and no scene.
26. set_time on an unknown clip returns ERR_STATE, with a NaN time ERR_INVALID_ARG; add_clip with a time that is not finite or with times
    that do not ascend strictly returns ERR_INVALID_ARG.  clear_clips makes ids start at 0 again and keeps the pose.
27. set_bones_from(skeleton) returns ERR_STATE before the skeleton's first pose, for a model without a skin, and for a skin whose n_bones is
    not the skeleton's n_joints; otherwise it is set_bones with the skeleton's palette AS IT IS AT THE CALL: a pose set before the update
    does not reach the vertices.  A skeleton may be destroyed right after the call.
Device-sourced transforms, attached instances, blends and inverse kinematics (include/dxr_amd.h "Attached instances", "blending", "inverse
kinematics"; DESIGN.md "update == build, with attachments").  A binding is (skeleton OBJECT, joint, local or none, the count of that
skeleton's poses that the scene last applied); a skeleton counts its poses.
28. set_transforms_mem(host) is set_transforms; with device memory the floats, arguments, refusals and the STALE rule are the same.
    transforms() returns the floats held, pending or applied.
29. attach(first, skeleton, joints, locals | None) refuses a range beyond the instances (ERR_STATE) first, then a joint >= n_joints
    (ERR_INVALID_ARG); count 0 is a no-op.  A refused call changes nothing.
30. A successful attach stores the binding and changes no stored transform.  On an updatable scene it marks those instances pending and the
    scene stale; on an unbuilt scene it only stores.  Attaching again replaces the binding, and a call without locals clears the earlier
    local.  attachment(i) answers (skeleton, joint) or None.
31. A transform setter of either kind whose range (count > 0) holds an attached instance is ERR_STATE and changes nothing.
32. detach keeps the floats the last successful update or build gave the instance and marks nothing; detaching unattached instances is a
    no-op; a range beyond the instances is ERR_STATE.
33. Posing a skeleton, by any of its producers, touches no scene: a fresh scene stays fresh and readable.  The next update of a scene with
    an instance attached to that skeleton is nevertheless a real update: pending() then holds "poses".
34. A successful update or build gives EVERY attached instance, hidden ones too, compose(W[joint], local), or W[joint] bit for bit without a
    local; W is the skeleton's joints as they are at the update, not at the attach.  A composed transform whose twelve floats are the
    identity's is the identity for everything downstream (the fresh build is handed the floats and decides as the update did).
35. update or build with an attachment to a skeleton that has never been posed is ERR_STATE and keeps everything pending, also together
    with rule 12.
36. A binding refers to the skeleton object, not to its slot: after "destroy right behind set_bones_from" the attached instances keep
    following nobody, poses of the replacement do not move them, and attachment(i) still answers the old skeleton.
37. add_mask / clear_masks / num_masks: ids start at 0, clearing restarts them, the pose stays.
38. set_blend: return codes by skeleton_blend_cases.validate (2 - 6 ERR_INVALID_ARG, 7 - 9 ERR_STATE); a refusal leaves pose, joints and
    palette as they were; otherwise pose = blended(...), `current` being the pose held, posed as set_pose poses.
39. solve_ik: return codes by ik_cases.validate (2 - 7 ERR_INVALID_ARG, 8 ERR_STATE); otherwise pose = ik_cases.solved(parents, pose, the
    joints before the call, constraints), posed.
40. Each successful set_pose, set_time, set_blend and solve_ik counts as exactly one pose for rule 33; a refused one counts as none.
Vertex arithmetic is that of skin_cases.skinned, deform_cases.normals_of, morph_cases.morphed, skeleton_cases.posed, skeleton_cases.sampled,
skeleton_cases.compose, skeleton_blend_cases.blended and ik_cases.solved, each held byte for byte to its kernel by the feature's own tests."""
import numpy as np

from deform_cases import normals_of
from morph_cases import morphed
import ik_cases
import skeleton_blend_cases
from skeleton_cases import compose, posed, sampled
from skin_cases import canonical_nans, skinned

OK, ERR_INVALID_ARG, ERR_STATE = 0, -1, -4
UNBUILT, FRESH, STALE = "never built since the last add", "fresh", "stale"
VERTEX = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3)])          # include/dxr_amd_types.h rt_vertex: 24 bytes
MAX_INFLUENCES, MAX_BONES, MAX_TARGETS = 8, 65536, 65536
IDENTITY = None                                                             # an instance transform: None, or float32[12] (3x4 row major)
IDENTITY_FLOATS = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def floats_of(x):
    """the twelve floats of an instance transform"""
    return IDENTITY_FLOATS if x is None else np.asarray(x, np.float32).reshape(12)


def is_identity(x):
    """the floats are the identity's (rule 34): what makes a one-instance scene single-level"""
    return x is None or bool(np.array_equal(floats_of(x), IDENTITY_FLOATS))


class Model:
    def __init__(self, verts, idx):
        self.verts = np.array(verts, VERTEX, copy=True).reshape(-1)
        self.idx = np.array(idx, np.uint32, copy=True).reshape(-1, 3)
        self.skin = None                # or dict(rest=VERTEX[V], bones=uint32[V, K], weights=float32[V, K], n_bones=int)
        self.morph = None               # or dict(base=VERTEX[V], offsets=uint32[T + 1], indices=uint32[E], dpos=float32[E, 3], dnrm=float32[E, 3] or None)
        self.scenes = []                # the scenes that hold the model

    # ---- the four vertex setters: rules 4, 6, 7, 15
    def _range(self, first, count):
        return OK if first <= len(self.verts) and count <= len(self.verts) - first else ERR_STATE

    def _changed(self):
        for s in self.scenes:
            if s.state != UNBUILT:
                s.state = STALE
                s.pending_models.add(id(self))

    def set_vertices(self, first, part):
        part = np.asarray(part, VERTEX).reshape(-1)
        if self._range(first, len(part)) != OK:
            return ERR_STATE
        if len(part) == 0:
            return OK
        self.verts[first:first + len(part)] = part
        self._changed()
        return OK

    def set_positions(self, first, xyz):
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        if self._range(first, len(xyz)) != OK:
            return ERR_STATE
        if len(xyz) == 0:
            return OK
        self.verts["position"][first:first + len(xyz)] = xyz
        self._changed()
        return OK

    def recompute_normals(self):
        self.verts["normal"] = normals_of(self.verts["position"], self.idx)
        self._changed()
        return OK

    # ---- skins: rules 5, 8, 9, 14, 15
    def set_skin(self, bones, weights, n_bones):
        bones = np.asarray(bones).reshape(len(self.verts), -1)
        k = bones.shape[1]
        if not 1 <= k <= MAX_INFLUENCES or not 1 <= n_bones <= MAX_BONES or (bones >= n_bones).any():
            return ERR_INVALID_ARG
        self.skin = dict(rest=self.verts.copy(), bones=bones.astype(np.uint32), weights=np.array(weights, np.float32).reshape(bones.shape), n_bones=int(n_bones))
        return OK

    def clear_skin(self):
        self.skin = None
        return OK

    def set_bones(self, palette):
        if self.skin is None:
            return ERR_STATE
        palette = np.asarray(palette, np.float32).reshape(-1, 12)
        assert len(palette) == self.skin["n_bones"]
        self.verts[:] = skinned(self.skin["rest"], self.skin["bones"], self.skin["weights"], palette)
        self._changed()
        return OK

    def set_bones_from(self, skeleton):                    # rule 27
        if skeleton.palette is None or self.skin is None or self.skin["n_bones"] != len(skeleton.parents):
            return ERR_STATE
        return self.set_bones(skeleton.palette)

    # ---- morph targets: rules 17 - 24
    def set_morph_targets(self, offsets, indices, dpos, dnrm=None):
        off = np.asarray(offsets, np.int64).reshape(-1)
        idx = np.asarray(indices, np.int64).reshape(-1)
        if len(off) - 1 > MAX_TARGETS or off[0] != 0 or (np.diff(off) < 0).any() or (idx[:off[-1]] >= len(self.verts)).any():
            return ERR_INVALID_ARG                             # rule 18
        for t in range(len(off) - 1):
            if (np.diff(idx[off[t]:off[t + 1]]) <= 0).any():
                return ERR_INVALID_ARG
        base = self.verts if self.skin is None else self.skin["rest"]
        self.morph = dict(base=base.copy(), offsets=off.astype(np.uint32), indices=idx.astype(np.uint32), dpos=np.array(dpos, np.float32).reshape(-1, 3),
                          dnrm=None if dnrm is None else np.array(dnrm, np.float32).reshape(-1, 3))
        return OK

    def clear_morph_targets(self):                         # rule 19
        self.morph = None
        return OK

    def set_morph_weights(self, weights):
        if self.morph is None:
            return ERR_STATE                                   # rule 20
        mo = self.morph
        out = morphed(mo["base"], mo["offsets"], mo["indices"], mo["dpos"], mo["dnrm"], weights)
        if self.skin is not None:
            self.skin["rest"] = out                            # rule 22: nothing a scene reads has changed
            return OK
        self.verts[:] = out                                    # rule 21
        self._changed()
        return OK

    def geometry(self):                 # rule 16
        return self.verts

    def skin_query(self):
        """(influences, bones) as rt_model_get_skin answers"""
        return (0, 0) if self.skin is None else (self.skin["bones"].shape[1], self.skin["n_bones"])

    def morph_query(self):
        """(targets, entries, has normal deltas) as rt_model_get_morph_targets answers"""
        mo = self.morph
        return (0, 0, False) if mo is None else (len(mo["offsets"]) - 1, int(mo["offsets"][-1]), mo["dnrm"] is not None)


class Skeleton:                         # rules 25, 26
    def __init__(self, parents, inverse_bind):
        self.parents = np.array(parents, np.int32, copy=True).reshape(-1)
        self.inverse_bind = np.array(inverse_bind, np.float32, copy=True).reshape(-1, 12)
        self.pose = self.joints = self.palette = None       # float32[n, 10], [n, 12], [n, 12] once posed
        self.clips = []                                     # [(times float32[K], keys float32[K, n, 10])]; the id is the place
        self.masks = []                                     # [float32[n]]; the id is the place (rule 37)
        self.poses = 0                                      # how many times it has been posed (rule 40)
        self.uid = None                                     # which skeleton object this is: World numbers them as they are made (rule 36)

    def set_pose(self, trs):
        self.pose = np.array(trs, np.float32, copy=True).reshape(len(self.parents), 10)
        self.joints, self.palette = posed(self.parents, self.inverse_bind, self.pose)
        self.poses += 1
        return OK

    def add_mask(self, weights):                        # rule 37
        self.masks.append(np.array(weights, np.float32, copy=True).reshape(len(self.parents)))
        return OK

    def clear_masks(self):
        self.masks = []
        return OK

    def num_masks(self):
        return len(self.masks)

    def set_blend(self, layers):
        """layers: [(clip or None for the current pose, time, weight, mask or None, mode)]: rule 38"""
        B = skeleton_blend_cases
        records = [(B.CURRENT_POSE if c is None else c, t, w, B.NO_MASK if m is None else m, mode) for c, t, w, m, mode in layers]
        what = B.validate(records, len(self.clips), len(self.masks), self.pose is not None)[0]
        if what:
            return ERR_INVALID_ARG if what <= 6 else ERR_STATE
        return self.set_pose(B.blended(self.clips, self.masks, layers, current=self.pose))

    def solve_ik(self, constraints):
        """constraints: [(kind, joint, target, pole, weight)]: rule 39"""
        what = ik_cases.validate(constraints, self.parents, self.pose is not None)[0]
        if what:
            return ERR_INVALID_ARG if what <= 7 else ERR_STATE
        return self.set_pose(ik_cases.solved(self.parents, self.pose, self.joints, constraints))

    def add_clip(self, times, keys):
        times = np.asarray(times, np.float32).reshape(-1)
        if len(times) == 0 or not np.isfinite(times).all() or (np.diff(times) <= 0).any():
            return ERR_INVALID_ARG
        self.clips.append((times.copy(), np.array(keys, np.float32, copy=True).reshape(len(times), len(self.parents), 10)))
        return OK

    def clear_clips(self):
        self.clips = []
        return OK

    def set_time(self, clip, t):
        if np.isnan(np.float32(t)):
            return ERR_INVALID_ARG
        if not 0 <= clip < len(self.clips):
            return ERR_STATE
        return self.set_pose(sampled(self.clips[clip][0], self.clips[clip][1], t))

    def snapshot(self):
        return (self.parents.tobytes(), self.inverse_bind.tobytes(), [(t.tobytes(), k.tobytes()) for t, k in self.clips], self.readers(),
                [m.tobytes() for m in self.masks], self.poses, self.uid)

    def readers(self):
        """what read_pose, read_joints and read_palette return, NaNs canonical; None before the first pose"""
        return None if self.pose is None else tuple(canonical_nans(a).tobytes() for a in (self.pose, self.joints, self.palette))


class Scene:
    def __init__(self, models):
        self.models = models            # the world's list of Model
        self.inst = []                  # [(model index, transform)]
        self.masks = []                 # one byte per instance
        self.state = UNBUILT
        self.pending_xforms = set()     # instances whose transform was set since the last successful update / build
        self.pending_masks = False      # a setter flipped some instance's visibility since then
        self.pending_models = set()     # id() of the models whose vertices were set since then
        self.applied_vis = None         # the visible sub-list the TLAS stands for
        self.att = {}                   # instance -> dict(sk=Skeleton, joint=int, local=float32[12] or None,
        #                                                   seen=the skeleton's poses at the last apply, or None)

    def add_model(self, mi, xform=IDENTITY):
        self.inst.append((mi, xform))
        self.masks.append(0xFF)
        if self not in self.models[mi].scenes:
            self.models[mi].scenes.append(self)
        self.state = UNBUILT            # rule 1: whatever was pending is what the build reads anyway
        self._clear_pending()
        return OK

    def _clear_pending(self):
        self.pending_xforms = set()
        self.pending_masks = False
        self.pending_models = set()

    def _range(self, first, count):
        return OK if first <= len(self.inst) and count <= len(self.inst) - first else ERR_STATE

    def set_transforms(self, first, xforms):
        if self._range(first, len(xforms)) != OK:
            return ERR_STATE
        if any(first + k in self.att for k in range(len(xforms))):
            return ERR_STATE                                   # rule 31
        for k, x in enumerate(xforms):
            self.inst[first + k] = (self.inst[first + k][0], None if x is None else np.array(x, np.float32).reshape(12))
        if xforms and self.state != UNBUILT:                   # rules 1, 2, 6
            self.state = STALE
            self.pending_xforms.update(range(first, first + len(xforms)))
        return OK

    def set_transform(self, i, x):
        return self.set_transforms(i, [x]) if i < len(self.inst) else ERR_STATE

    def set_transforms_mem(self, first, xforms, mem):       # rule 28: where the floats come from changes nothing
        assert mem in ("host", "device")
        return self.set_transforms(first, xforms)

    def transforms(self):
        """float32[n, 12]: the floats held, pending or applied"""
        return np.array([floats_of(x) for _, x in self.inst], np.float32).reshape(-1, 12)

    def attach(self, first, skeleton, joints, locals=None):  # rules 29, 30
        joints = [int(j) for j in np.asarray(joints).reshape(-1)]
        if self._range(first, len(joints)) != OK:
            return ERR_STATE
        if any(j >= len(skeleton.parents) for j in joints):
            return ERR_INVALID_ARG
        for k, j in enumerate(joints):
            local = None if locals is None else np.array(np.asarray(locals, np.float32).reshape(-1, 12)[k], np.float32, copy=True)
            self.att[first + k] = dict(sk=skeleton, joint=j, local=local, seen=None)
        if joints and self.state != UNBUILT:
            self.state = STALE
            self.pending_xforms.update(range(first, first + len(joints)))
        return OK

    def detach(self, first, count):                         # rule 32
        if self._range(first, count) != OK:
            return ERR_STATE
        for i in range(first, first + count):
            self.att.pop(i, None)
        return OK

    def attachment(self, i):
        a = self.att.get(i)
        return None if a is None else (a["sk"], a["joint"])

    def unposed(self):
        """an instance is attached to a skeleton that has never been posed (rule 35)"""
        return any(a["sk"].pose is None for a in self.att.values())

    def posed_since(self):
        """the attached instances whose skeleton has been posed since the scene last applied it (rule 33)"""
        return sorted(i for i, a in self.att.items() if a["sk"].pose is not None and a["seen"] != a["sk"].poses)

    def set_masks(self, first, masks):
        masks = [int(m) & 0xFF for m in masks]
        if self._range(first, len(masks)) != OK:
            return ERR_STATE
        flips = any((self.masks[first + k] != 0) != (m != 0) for k, m in enumerate(masks))
        self.masks[first:first + len(masks)] = masks
        if flips and self.state != UNBUILT:                    # rules 1, 3
            self.state = STALE
            self.pending_masks = True
        return OK

    def set_mask(self, i, m):
        return self.set_masks(i, [m]) if i < len(self.inst) else ERR_STATE

    def visible(self):
        return [k for k, m in enumerate(self.masks) if m]

    def pending(self):
        """the kinds of edit the next update applies: a subset of {"transforms", "masks", "vertices", "poses"}"""
        kinds = set()
        if self.pending_xforms:
            kinds.add("transforms")
        if self.pending_masks:
            kinds.add("masks")
        if self.pending_models:
            kinds.add("vertices")
        if self.posed_since():
            kinds.add("poses")
        return frozenset(kinds)

    def update(self):
        """-> (code, what was applied: None when refused, frozenset() for the no-op of rule 11)"""
        if self.state == UNBUILT:
            return ERR_STATE, None                             # rule 1
        kinds = self.pending()
        if not kinds:
            return OK, kinds                                   # rule 11
        if not self.visible() or self.unposed():
            return ERR_STATE, None                             # rules 12, 35: everything pending kept
        self._applied()
        return OK, kinds

    def build(self):
        if not self.inst:
            return ERR_INVALID_ARG, None
        if not self.visible() or self.unposed():
            return ERR_STATE, None                             # rules 12, 35
        kinds = self.pending()
        self._applied(everything=True)
        return OK, kinds

    def _applied(self, everything=False):
        for i, a in self.att.items():                          # rule 34: W as it is now; an instance that has seen this pose holds its floats already
            if not everything and a["seen"] == a["sk"].poses:
                continue
            w = a["sk"].joints[a["joint"]]
            x = w.copy() if a["local"] is None else compose(w, a["local"])[0]
            self.inst[i] = (self.inst[i][0], np.array(x, np.float32).reshape(12))
            a["seen"] = a["sk"].poses
        self._clear_pending()
        self.state = FRESH
        self.applied_vis = self.visible()

    def readable(self):                 # rule 13
        return self.state == FRESH


class World:
    """models and scenes, and a version that moves with every change of state: two equal versions are the same state"""

    def __init__(self):
        self.models, self.scenes, self.skeletons = [], [], []
        self.made = 0                   # skeleton objects made so far: the next one's uid

    def add_model(self, verts, idx):
        self.models.append(Model(verts, idx))
        return len(self.models) - 1

    def add_skeleton(self, parents, inverse_bind):
        self.skeletons.append(self._skeleton(parents, inverse_bind))
        return len(self.skeletons) - 1

    def _skeleton(self, parents, inverse_bind):
        sk = Skeleton(parents, inverse_bind)
        sk.uid, self.made = self.made, self.made + 1
        return sk

    def replace_skeleton(self, k):
        """the skeleton of slot k is destroyed; a new one of the same joints, never posed, without clips or masks, takes the slot.  Scenes
        that hold instances attached to the old one keep it (rule 36)"""
        old = self.skeletons[k]
        self.skeletons[k] = self._skeleton(old.parents, old.inverse_bind)

    def add_scene(self):
        self.scenes.append(Scene(self.models))
        return len(self.scenes) - 1

    def snapshot(self):
        """everything a refusal must leave as it was (rule 10), comparable with =="""
        def morph(mo):
            return None if mo is None else (mo["base"].tobytes(), mo["offsets"].tobytes(), mo["indices"].tobytes(), mo["dpos"].tobytes(), None if mo["dnrm"] is None else mo["dnrm"].tobytes())
        return ([(m.verts.tobytes(), None if m.skin is None else (m.skin["rest"].tobytes(), m.skin["bones"].tobytes(), m.skin["weights"].tobytes(), m.skin["n_bones"]), morph(m.morph))
                 for m in self.models], [k.snapshot() for k in self.skeletons],
                [([(mi, None if x is None else np.asarray(x, np.float32).tobytes()) for mi, x in s.inst], list(s.masks), s.state, sorted(s.pending_xforms),
                  s.pending_masks, len(s.pending_models),
                  sorted((i, a["sk"].uid, a["sk"].poses, a["joint"], None if a["local"] is None else a["local"].tobytes(), a["seen"])
                         for i, a in s.att.items()))
                 for s in self.scenes], self.made)

    def readers(self):
        """what the library's readers can return of the state -- geometry(), the skin and morph queries, masks(), whether a scene is readable,
        a posed skeleton's arrays and its mask count, a scene's transforms() and attachments -- and nothing of the hidden arrays: the rest
        pose and the morph base, the local matrices and what a scene has seen of a skeleton's poses"""
        return ([(m.verts.tobytes(), m.skin_query(), m.morph_query()) for m in self.models], [(k.readers(), k.num_masks()) for k in self.skeletons],
                [(list(s.masks), s.state, s.transforms().tobytes(), [a and (a[0].uid, a[1]) for a in map(s.attachment, range(len(s.inst)))])
                 for s in self.scenes])
