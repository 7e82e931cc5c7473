#!/usr/bin/env python3
"""What rt_scene_update costs on the flagship two-level scene (C4: scenes.instance_grid(64) = 4096 instances of two meshes), against the only
thing an application could do before it existed: a new scene, 4096 x add_model of already-built models, rt_scene_build, set_scene.

  python3 tools/tlas_update_timing.py [--updates N] [--warmup W] [--frames] [--baseline-only]

Every step turns the instances one more degree about y.  Per step, alternating (so that drift hits all alike): the baseline, then an update
with all 4096 transforms pending, with 64 consecutive ones, with one.  Wall clock = host time from the first setter (baseline: from
rt_scene_create) to a context synchronise behind the update (build + set_scene); update_ms / build_ms = the library's device events.  Medians
and quartiles over N >= 20 steps after W warm-up steps.  GATE: the all-pending update's median wall clock is no worse than the baseline's
plus twice the baseline's interquartile range.  --frames adds the price of the dropped shadow cache on the 4K realtime pipeline: the first
frame after an update against the steady frames before it.  --baseline-only runs on a library without the update calls (the parent commit's,
named by DXR_AMD_LIB), for the same figures from the code as it stood."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from dxrexperiments_amd import capi, rtypes as T, scenes  # noqa: E402


def turned(xf, degrees):
    """every transform's linear part turned about the world's y axis (rigid: the grid positions stay)"""
    a = np.deg2rad(degrees)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    m = xf.astype(np.float64).reshape(-1, 3, 4).copy()
    m[:, :, :3] = np.einsum("ij,njk->nik", ry, m[:, :, :3])
    return np.ascontiguousarray(m.reshape(-1, 12).astype(np.float32))


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return med, q3 - q1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    assert args.updates >= 20, "at least 20 timed steps"
    if args.baseline_only:                     # (a library from before the update calls: bind what it has)
        for name in ("rt_scene_set_instance_transform", "rt_scene_set_instance_transforms", "rt_scene_update", "rt_scene_update_ms"):
            capi.SIGNATURES.pop(name, None)
    ctx = capi.Context(0)
    sus = capi.Model(ctx, path=os.path.join(ROOT, "tests", "golden", "susanne.obj"))
    blob = capi.Model(ctx, *scenes.blob_mesh(level=3))
    xf0 = scenes.instance_grid(64)
    n = xf0.shape[0]
    models = [sus if k % 2 == 0 else blob for k in range(n)]
    W, H = 3840, 2160
    pipe = capi.Pipeline(ctx, capi.PIPELINE_REALTIME)
    r = np.random.default_rng(5)
    for k in range(n):
        m = T.default_material()
        m["albedo"][:3] = r.uniform(0.1, 0.9, 3)
        m["type"] = k % 3
        pipe.add_material(m)
    pipe.set_environment_cube(scenes.sky_cubemap(32))
    pipe.create_output(W, H)

    def fresh_scene(xf):
        sc = capi.Scene(ctx)
        for k in range(n):
            sc.add_model(models[k], xf[k])
        sc.build()
        return sc

    scene = fresh_scene(xf0)                   # (builds the two BLASes: every later build finds them built)
    pipe.set_scene(scene)
    ctx.synchronize()
    steps = args.warmup + args.updates
    poses = [turned(xf0, s + 1) for s in range(steps + 8)]
    wall = {"baseline": [], "all": [], "64": [], "1": []}
    dev = {"baseline": [], "all": [], "64": [], "1": []}
    keep = None
    for s in range(steps):
        xf = poses[s]
        t0 = time.perf_counter()
        sc = fresh_scene(xf)
        pipe.set_scene(sc)
        ctx.synchronize()
        t1 = time.perf_counter()
        if s >= args.warmup:
            wall["baseline"].append((t1 - t0) * 1e3)
            dev["baseline"].append(sc.build_ms())
        if keep is not None:
            keep.close()
        keep = sc
        if args.baseline_only:
            continue
        for name, first, count in (("all", 0, n), ("64", 2000, 64), ("1", 2000, 1)):
            t0 = time.perf_counter()
            if count == 1:
                scene.set_transform(first, xf[first])
            else:
                scene.set_transforms(first, xf[first:first + count])
            scene.update()
            ctx.synchronize()
            t1 = time.perf_counter()
            if s >= args.warmup:
                wall[name].append((t1 - t0) * 1e3)
                dev[name].append(scene.update_ms())
    print("scene: scenes.instance_grid(64), %d instances of susanne.obj and blob_mesh(level=3); %d timed steps after %d warm-up steps" % (n, args.updates, args.warmup))
    print("%-34s %12s %12s %14s" % ("", "wall ms", "wall IQR", "device ms"))
    rows = (("baseline", "new scene + 4096 add_model + build + set_scene"),) if args.baseline_only else \
           (("baseline", "new scene + add_model + build + set"), ("all", "update, 4096 pending"), ("64", "update, 64 pending"), ("1", "update, 1 pending"))
    stats = {}
    for key, label in rows:
        med, iqr = quartiles(wall[key])
        dmed, _ = quartiles(dev[key])
        stats[key] = (med, iqr, dmed)
        print("%-34s %12.3f %12.3f %14.3f" % (label, med, iqr, dmed))
    ok = True
    if not args.baseline_only:
        base, iqr, _ = stats["baseline"]
        ok = stats["all"][0] <= base + 2.0 * iqr
        print("GATE all-pending update wall %.3f ms <= baseline %.3f ms + 2 x IQR %.3f ms: %s" % (stats["all"][0], base, iqr, "PASS" if ok else "FAIL"))
        print("update with 64 pending / all pending: wall %.2f, device %.2f;  1 pending / all pending: wall %.2f, device %.2f"
              % (stats["64"][0] / stats["all"][0], stats["64"][2] / stats["all"][2], stats["1"][0] / stats["all"][0], stats["1"][2] / stats["all"][2]))
    if args.frames and not args.baseline_only:
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
            scene.set_transforms(0, poses[steps + s])
            scene.update()
            first.append(frame())
        sm, si = quartiles(steady)
        fm, fi = quartiles(first)
        print("4K realtime frame, wall: steady %.3f ms (IQR %.3f, %d frames); first frame after an update %.3f ms (IQR %.3f, %d frames): the dropped shadow cache and "
              "primary-mode samples cost %.3f ms" % (sm, si, len(steady), fm, fi, len(first), fm - sm))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
