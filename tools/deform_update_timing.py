#!/usr/bin/env python3
"""What a deforming update costs (rt_model_set_vertices + rt_scene_update), against the only route to the same scene before it existed: a new
rt_model from host arrays (upload, every BLAS buffer allocated), a new scene, add_model for every instance, rt_scene_build.

  python3 tools/deform_update_timing.py [--updates N] [--warmup W] [--frames]

Two scenes: (1) the bench scene, scenes.sponza_class() (~262 k triangles), one identity instance, EVERY vertex displaced each step;
(2) C4, scenes.instance_grid(64) = 4096 instances of susanne.obj and a blob, the blob (2048 instances) deformed each step.  Per step,
alternating (so that drift hits both alike): the old route, then the update with the vertices coming from a host array and from device
memory.  Wall clock = host time from the first call to a context synchronise behind the last; update_ms / build_ms = the library's device
events.  (2) also times an update with one transform pending and no vertices (the TLAS share: rt_update_tlas alone), so that the BLAS share
of a deforming update is the difference.  Medians and interquartile ranges over N >= 20 steps after W warm-up steps.  --frames adds the first
4K realtime frame after a deforming update against the steady frames before it (the dropped shadow cache).  Nothing here gates: the figures
are recorded."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from dxrexperiments_amd import capi, rtypes as T, scenes  # noqa: E402


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return med, q3 - q1


def moved(verts, step, amount):
    """every vertex displaced along a wave through the mesh (deterministic per step)"""
    out = verts.copy()
    p = verts["position"].astype(np.float64)
    out["position"] = (p + amount * np.sin(0.37 * step + 3.0 * p[:, [1, 2, 0]])).astype(np.float32)
    return out


def report(title, rows, wall, dev):
    print(title)
    print("%-58s %12s %12s %14s" % ("", "wall ms", "wall IQR", "device ms"))
    for key, label in rows:
        med, iqr = quartiles(wall[key])
        dmed, _ = quartiles(dev[key])
        print("%-58s %12.3f %12.3f %14.3f" % (label, med, iqr, dmed))


def run(ctx, meshes, inst, deform_model, amount, steps, warmup, extra_transform=False):
    """meshes: [(verts, idx)]; inst: [(model, xform)]; the model `deform_model` changes every step"""
    gm = [capi.Model(ctx, v, i) for v, i in meshes]
    scene = capi.Scene(ctx)
    for mi, x in inst:
        scene.add_model(gm[mi], x)
    scene.build()
    ctx.synchronize()
    v0, idx = meshes[deform_model]
    keys = ["old", "host", "device"] + (["tlas"] if extra_transform else [])
    wall = {k: [] for k in keys}
    dev = {k: [] for k in keys}
    keep = None
    for s in range(warmup + steps):
        new = moved(v0, s + 1, amount)
        dbuf = ctx.upload(new)                           # (the producer's output: not part of what is timed)
        ctx.synchronize()
        t0 = time.perf_counter()
        fresh_model = capi.Model(ctx, new, idx)
        sc = capi.Scene(ctx)
        for mi, x in inst:
            sc.add_model(fresh_model if mi == deform_model else gm[mi], x)
        sc.build()
        ctx.synchronize()
        t1 = time.perf_counter()
        took = {"old": ((t1 - t0) * 1e3, sc.build_ms())}
        if keep is not None:
            keep[0].close(); keep[1].close()
        keep = (sc, fresh_model)
        t0 = time.perf_counter()
        gm[deform_model].set_vertices(new)
        scene.update()
        ctx.synchronize()
        took["host"] = ((time.perf_counter() - t0) * 1e3, scene.update_ms())
        t0 = time.perf_counter()
        gm[deform_model].set_vertices_device(dbuf.ptr, len(new))
        scene.update()
        ctx.synchronize()
        took["device"] = ((time.perf_counter() - t0) * 1e3, scene.update_ms())
        if extra_transform:
            t0 = time.perf_counter()
            scene.set_transform(7, inst[7][1])
            scene.update()
            ctx.synchronize()
            took["tlas"] = ((time.perf_counter() - t0) * 1e3, scene.update_ms())
        dbuf.close()
        if s >= warmup:
            for k, (w, d) in took.items():
                wall[k].append(w); dev[k].append(d)
    if keep is not None:
        keep[0].close(); keep[1].close()
    return scene, gm, wall, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", action="store_true")
    args = ap.parse_args()
    assert args.updates >= 20, "at least 20 timed steps"
    ctx = capi.Context(0)

    v, idx = scenes.sponza_class()
    scene, gm, wall, dev = run(ctx, [(v, idx)], [(0, None)], 0, 0.05, args.updates, args.warmup)
    report("bench scene: scenes.sponza_class(), %d triangles, %d vertices, one identity instance, every vertex displaced; %d timed steps after %d"
           % (len(idx), len(v), args.updates, args.warmup),
           (("old", "new model from host arrays + new scene + rt_scene_build"), ("host", "set_vertices (host array) + rt_scene_update"),
            ("device", "set_vertices (device memory) + rt_scene_update")), wall, dev)
    scene.close(); gm[0].close()

    sus = capi.Model(ctx, path=os.path.join(ROOT, "tests", "golden", "susanne.obj")).geometry()
    blob = scenes.blob_mesh(level=3)
    xf = scenes.instance_grid(64)
    inst = [(k % 2, xf[k]) for k in range(xf.shape[0])]
    scene, gm, wall, dev = run(ctx, [sus, blob], inst, 1, 0.1, args.updates, args.warmup, extra_transform=True)
    report("C4: scenes.instance_grid(64), %d instances of susanne.obj (%d triangles) and blob_mesh(level=3) (%d triangles), the blob deformed"
           % (len(inst), len(sus[1]), len(blob[1])),
           (("old", "new blob model + new scene + 4096 add_model + rt_scene_build"), ("host", "set_vertices (host array) + rt_scene_update"),
            ("device", "set_vertices (device memory) + rt_scene_update"), ("tlas", "one transform pending, no vertices: the TLAS share")), wall, dev)
    d_all, d_tlas = quartiles(dev["device"])[0], quartiles(dev["tlas"])[0]
    print("deforming update, device: %.3f ms, of which the records + world boxes + TLAS of a rigid update with 1 pending are %.3f ms; the BLAS rebuild and the "
          "2048 instances' world boxes: %.3f ms" % (d_all, d_tlas, d_all - d_tlas))

    if args.frames:
        W, H = 3840, 2160
        pipe = capi.Pipeline(ctx, capi.PIPELINE_REALTIME)
        r = np.random.default_rng(5)
        for k in range(len(inst)):
            m = T.default_material()
            m["albedo"][:3] = r.uniform(0.1, 0.9, 3)
            m["type"] = k % 3
            pipe.add_material(m)
        pipe.set_environment_cube(scenes.sky_cubemap(32))
        pipe.create_output(W, H)
        pipe.set_scene(scene)
        host = capi.ProgressiveHost(4)
        cam = capi.camera_array((0.0, 30.0, 110.0), (0.0, 0.0, 0.0), (0, 1, 0), 0.9, W / H)
        f = 0

        def frame():
            nonlocal f
            f += 1
            pipe.update(host.update_realtime(cam, 0.0, f, W, H))
            t0 = time.perf_counter()
            pipe.render()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(6):
            frame()
        steady, first = [], []
        for s in range(8):
            steady += [frame() for _ in range(4)]
            gm[1].set_vertices(moved(blob[0], 100 + s, 0.1))
            scene.update()
            first.append(frame())
        sm, si = quartiles(steady)
        fm, fi = quartiles(first)
        print("4K realtime frame, wall: steady %.3f ms (IQR %.3f, %d frames); first frame after a deforming update %.3f ms (IQR %.3f, %d frames): the dropped "
              "shadow cache and primary-mode samples cost %.3f ms" % (sm, si, len(steady), fm, fi, len(first), fm - sm))
        pipe.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
