#!/usr/bin/env python3
"""What a skinned update costs (rt_model_set_bones + rt_scene_update), against the only route to the same scene before it existed:
rt_model_set_vertices from a host array of finished vertices + rt_scene_update (and the same route from a device array).

  python3 tools/skin_update_timing.py [--updates N] [--warmup W] [--repeats R]

Two scenes, those of tools/deform_update_timing.py: (1) the bench scene, scenes.sponza_class() (~262 k triangles), one identity instance;
(2) C4, scenes.instance_grid(64) = 4096 instances of susanne.obj and a blob, the blob (2048 instances) animated.  The animated mesh has a
skin of K = 4 influences over 64 bones (slabs along y, weights falling off to the neighbouring slabs); every step poses every bone anew.
(a) Per step, alternating (so that drift hits both alike): set_vertices from a host array of the finished vertices + update, the same from
device memory, set_bones from a host palette + update.  Wall clock = host time from the first call to a context synchronise behind the
last; device ms = rt_scene_update_ms.  What the host spends on PRODUCING the finished vertices (here: numpy, fp32, vectorised) is reported on
a line of its own and is part of no other figure.
(b) The kernel alone: R back-to-back rt_model_set_bones calls with the palette in device memory between two events on the context's stream,
against R back-to-back rt_model_set_vertices calls from device memory (a device-to-device copy of the same vertex array: the yardstick of a
kernel that should be bound by the same bytes plus the skin's), for 64 bones and, for the two palette paths at their edge, RT_SKIN_LDS_BONES
(staged into LDS) and RT_SKIN_LDS_BONES + 1 (gathered from global memory).  The figures include the gaps between back-to-back launches.
Medians and interquartile ranges over N >= 20 steps after W warm-up steps.  Nothing here gates: the figures are recorded."""
import argparse
import ctypes as C
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from dxrexperiments_amd import capi, rtypes as T, scenes  # noqa: E402


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return med, q3 - q1


def lds_bones():
    text = open(os.path.join(ROOT, "dxrexperiments_amd", "csrc", "rt_skin.h")).read()
    return int(re.search(r"^#define RT_SKIN_LDS_BONES (\d+)", text, flags=re.M).group(1))


def slab_skin(verts, n_bones, k=4):
    """bone b owns the b-th slab of the mesh along y; a vertex is held by its slab and the k - 1 slabs after it (clamped), with weights that
    fall off and sum to 1"""
    y = verts["position"][:, 1].astype(np.float64)
    t = (y - y.min()) / max(y.max() - y.min(), 1e-30) * n_bones
    own = np.clip(t.astype(np.int64), 0, n_bones - 1)
    bones = np.clip(own[:, None] + np.arange(k)[None, :], 0, n_bones - 1).astype(np.uint32)
    w = 0.5 ** np.arange(k)[None, :] * np.ones((len(verts), 1))
    return bones, (w / w.sum(axis=1, keepdims=True)).astype(np.float32)


def palette_of(n_bones, step, centre):
    """every bone turned about y through `centre` by an angle that travels along the skeleton, and lifted a little"""
    a = 0.15 * np.sin(0.37 * step + 0.21 * np.arange(n_bones))
    m = np.zeros((n_bones, 3, 4))
    m[:, 0, 0] = np.cos(a); m[:, 0, 2] = np.sin(a)
    m[:, 1, 1] = 1.0
    m[:, 2, 0] = -np.sin(a); m[:, 2, 2] = np.cos(a)
    m[:, :, 3] = centre - np.einsum("bij,j->bi", m[:, :, :3], centre) + np.stack([0 * a, 0.02 * np.sin(a * 9), 0 * a], axis=1)
    return m.reshape(n_bones, 12).astype(np.float32)


def host_skinned(rest, bones, weights, palette):
    """the finished vertices as a host would make them (fp32, vectorised numpy; not the library's operation order: a stand-in for the
    caller's own skinning, timed on its own)"""
    B = np.einsum("vk,vke->ve", weights, palette[bones]).reshape(-1, 3, 4)
    out = rest.copy()
    out["position"] = np.einsum("vij,vj->vi", B[:, :, :3], rest["position"]) + B[:, :, 3]
    n = np.einsum("vij,vj->vi", B[:, :, :3], rest["normal"])
    d = np.sqrt((n * n).sum(axis=1, keepdims=True))
    out["normal"] = np.where(d > 0, n / np.where(d > 0, d, 1), 0)
    return out


class Events:
    """two events on the context's stream (the HIP runtime the library is linked with)"""

    def __init__(self, ctx):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p()
        capi._check(capi.lib().rt_context_get_stream(ctx.h, C.byref(self.stream)))
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def record(self, which):
        assert self.hip.hipEventRecord(self.e[which], self.stream) == 0

    def ms(self):
        out = C.c_float()
        assert self.hip.hipEventSynchronize(self.e[1]) == 0 and self.hip.hipEventElapsedTime(C.byref(out), self.e[0], self.e[1]) == 0
        return out.value

    def close(self):
        for e in self.e:
            self.hip.hipEventDestroy(e)


def updates(ctx, scene, model, rest, n_bones, steps, warmup):
    """(a): the three routes, alternating"""
    bones, weights = slab_skin(rest, n_bones)
    model.set_skin(bones, weights, n_bones)
    centre = 0.5 * (rest["position"].min(axis=0) + rest["position"].max(axis=0)).astype(np.float64)
    keys = ("verts_host", "verts_device", "bones_host")
    wall = {k: [] for k in keys}
    dev = {k: [] for k in keys}
    produce = []
    for s in range(warmup + steps):
        palette = palette_of(n_bones, s + 1, centre)
        t0 = time.perf_counter()
        new = host_skinned(rest, bones, weights, palette)
        t_produce = (time.perf_counter() - t0) * 1e3
        dbuf = ctx.upload(new)                           # (a device producer's output: not part of what is timed)
        ctx.synchronize()
        took = {}
        t0 = time.perf_counter()
        model.set_vertices(new)
        scene.update()
        ctx.synchronize()
        took["verts_host"] = ((time.perf_counter() - t0) * 1e3, scene.update_ms())
        t0 = time.perf_counter()
        model.set_vertices_device(dbuf.ptr, len(new))
        scene.update()
        ctx.synchronize()
        took["verts_device"] = ((time.perf_counter() - t0) * 1e3, scene.update_ms())
        t0 = time.perf_counter()
        model.set_bones(palette)
        scene.update()
        ctx.synchronize()
        took["bones_host"] = ((time.perf_counter() - t0) * 1e3, scene.update_ms())
        dbuf.close()
        if s >= warmup:
            produce.append(t_produce)
            for k, (w, d) in took.items():
                wall[k].append(w); dev[k].append(d)
    print("%-64s %12s %12s %14s" % ("", "wall ms", "wall IQR", "update_ms"))
    for key, label in (("verts_host", "set_vertices (host array of finished vertices) + rt_scene_update"),
                       ("verts_device", "set_vertices (device memory) + rt_scene_update"),
                       ("bones_host", "set_bones (host palette, %d bones) + rt_scene_update" % n_bones)):
        med, iqr = quartiles(wall[key])
        print("%-64s %12.3f %12.3f %14.3f" % (label, med, iqr, quartiles(dev[key])[0]))
    med, iqr = quartiles(produce)
    print("%-64s %12.3f %12.3f %14s" % ("producing the finished vertices on the host (numpy; in no figure above)", med, iqr, "-"))


def kernel_alone(ctx, model, rest, bone_counts, steps, warmup, repeats):
    """(b): the skin kernel against a device-to-device copy of the vertex array"""
    ev = Events(ctx)
    nv = len(rest)
    centre = 0.5 * (rest["position"].min(axis=0) + rest["position"].max(axis=0)).astype(np.float64)
    vbuf = ctx.upload(rest)

    def timed(call):
        out = []
        for s in range(warmup + steps):
            ctx.synchronize()
            ev.record(0)
            for _ in range(repeats):
                call()
            ev.record(1)
            ms = ev.ms() / repeats
            if s >= warmup:
                out.append(ms * 1e3)
        return quartiles(out)
    copy, copy_iqr = timed(lambda: model.set_vertices_device(vbuf.ptr, nv))
    print("%-64s %10.2f us (IQR %.2f): %.0f GB/s read + written" % ("device-to-device copy of %d vertices (%.2f MB)" % (nv, 24e-6 * nv), copy, copy_iqr,
                                                                 48e-3 * nv / copy))
    for n_bones in bone_counts:
        bones, weights = slab_skin(rest, n_bones)
        model.set_skin(bones, weights, n_bones)
        pbuf = ctx.upload(palette_of(n_bones, 1, centre))
        med, iqr = timed(lambda: model.set_bones_device(pbuf.ptr))
        moved = nv * (48 + 4 * 6) + ((nv + 255) // 256) * 48 * n_bones * (n_bones <= lds_bones())
        print("%-64s %10.2f us (IQR %.2f): %.2f x the copy; %.0f GB/s over vertices + skin%s"
              % ("k_skin_vertices, K = 4, %d bones (%s)" % (n_bones, "LDS" if n_bones <= lds_bones() else "global"), med, iqr, med / copy, 1e-3 * moved / med,
                 " + staging" if n_bones <= lds_bones() else ""))
        ctx.synchronize()
        pbuf.close()
    model.clear_skin()
    model.set_vertices(rest)
    vbuf.close()
    ev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=50)
    args = ap.parse_args()
    assert args.updates >= 20, "at least 20 timed steps"
    ctx = capi.Context(0)
    n_lds = lds_bones()

    v, idx = scenes.sponza_class()
    v = np.ascontiguousarray(v, T.VERTEX)
    model = capi.Model(ctx, v, idx)
    scene = capi.Scene(ctx)
    scene.add_model(model, None)
    scene.build()
    print("bench scene: scenes.sponza_class(), %d triangles, %d vertices, one identity instance; K = 4, 64 bones; %d timed steps after %d"
          % (len(idx), len(v), args.updates, args.warmup))
    updates(ctx, scene, model, v, 64, args.updates, args.warmup)
    print("the kernel alone, %d back-to-back calls per sample:" % args.repeats)
    kernel_alone(ctx, model, v, (64, n_lds, n_lds + 1), args.updates, args.warmup, args.repeats)
    scene.close(); model.close()

    sus = capi.Model(ctx, path=os.path.join(ROOT, "tests", "golden", "susanne.obj")).geometry()
    blob = scenes.blob_mesh(level=3)
    blob = (np.ascontiguousarray(blob[0], T.VERTEX), blob[1])
    xf = scenes.instance_grid(64)
    inst = [(k % 2, xf[k]) for k in range(xf.shape[0])]
    gm = [capi.Model(ctx, *sus), capi.Model(ctx, *blob)]
    scene = capi.Scene(ctx)
    for mi, x in inst:
        scene.add_model(gm[mi], x)
    scene.build()
    print("C4: scenes.instance_grid(64), %d instances of susanne.obj (%d triangles) and blob_mesh(level=3) (%d triangles, %d vertices), the blob animated"
          % (len(inst), len(sus[1]), len(blob[1]), len(blob[0])))
    updates(ctx, scene, gm[1], blob[0], 64, args.updates, args.warmup)
    scene.close()
    for m in gm:
        m.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
