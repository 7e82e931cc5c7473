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
Vertex arithmetic is that of skin_cases.skinned and deform_cases.normals_of, each held byte for byte to its kernel by the feature's own tests."""
import numpy as np

from deform_cases import normals_of
from skin_cases import skinned

OK, ERR_INVALID_ARG, ERR_STATE = 0, -1, -4
UNBUILT, FRESH, STALE = "never built since the last add", "fresh", "stale"
VERTEX = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3)])          # include/dxr_amd_types.h rt_vertex: 24 bytes
MAX_INFLUENCES, MAX_BONES = 8, 65536
IDENTITY = None                                                             # an instance transform: None, or float32[12] (3x4 row major)


class Model:
    def __init__(self, verts, idx):
        self.verts = np.array(verts, VERTEX, copy=True).reshape(-1)
        self.idx = np.array(idx, np.uint32, copy=True).reshape(-1, 3)
        self.skin = None                # or dict(rest=VERTEX[V], bones=uint32[V, K], weights=float32[V, K], n_bones=int)
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

    def geometry(self):                 # rule 16
        return self.verts


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
        for k, x in enumerate(xforms):
            self.inst[first + k] = (self.inst[first + k][0], None if x is None else np.array(x, np.float32).reshape(12))
        if xforms and self.state != UNBUILT:                   # rules 1, 2, 6
            self.state = STALE
            self.pending_xforms.update(range(first, first + len(xforms)))
        return OK

    def set_transform(self, i, x):
        return self.set_transforms(i, [x]) if i < len(self.inst) else ERR_STATE

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
        """the kinds of edit the next update applies: a subset of {"transforms", "masks", "vertices"}"""
        kinds = set()
        if self.pending_xforms:
            kinds.add("transforms")
        if self.pending_masks:
            kinds.add("masks")
        if self.pending_models:
            kinds.add("vertices")
        return frozenset(kinds)

    def update(self):
        """-> (code, what was applied: None when refused, frozenset() for the no-op of rule 11)"""
        if self.state == UNBUILT:
            return ERR_STATE, None                             # rule 1
        kinds = self.pending()
        if not kinds:
            return OK, kinds                                   # rule 11
        if not self.visible():
            return ERR_STATE, None                             # rule 12: everything pending kept
        self._applied()
        return OK, kinds

    def build(self):
        if not self.inst:
            return ERR_INVALID_ARG, None
        if not self.visible():
            return ERR_STATE, None                             # rule 12
        kinds = self.pending()
        self._applied()
        return OK, kinds

    def _applied(self):
        self._clear_pending()
        self.state = FRESH
        self.applied_vis = self.visible()

    def readable(self):                 # rule 13
        return self.state == FRESH


class World:
    """models and scenes, and a version that moves with every change of state: two equal versions are the same state"""

    def __init__(self):
        self.models, self.scenes = [], []

    def add_model(self, verts, idx):
        self.models.append(Model(verts, idx))
        return len(self.models) - 1

    def add_scene(self):
        self.scenes.append(Scene(self.models))
        return len(self.scenes) - 1

    def snapshot(self):
        """everything a refusal must leave as it was (rule 10), comparable with =="""
        return ([(m.verts.tobytes(), None if m.skin is None else (m.skin["rest"].tobytes(), m.skin["bones"].tobytes(), m.skin["weights"].tobytes(), m.skin["n_bones"]))
                 for m in self.models],
                [([(mi, None if x is None else np.asarray(x, np.float32).tobytes()) for mi, x in s.inst], list(s.masks), s.state, sorted(s.pending_xforms),
                  s.pending_masks, len(s.pending_models)) for s in self.scenes])
