#!/usr/bin/env python3
"""What a masked rt_scene_update costs on the flagship two-level scene (C4: scenes.instance_grid(64) = 4096 instances of two meshes), beside
what an application could do before instance masks existed: update the full list (it could not hide anything), or hide by building a second
scene of the instances that are left.

  python3 tools/instance_masks_timing.py [--updates N] [--warmup W] [--parent]

Per step, alternating in one process (so that drift hits all alike):
  full      one transform pending, nothing hidden                       (what the parent commit's library does too)
  rebuild   a new scene of the visible half + add_model + rt_scene_build (the parent's only way to hide)
  half      the odd instances hidden + the same transform pending, one update
  quarter   a quarter of the pool shown again (every fourth instance), one update
and, to come back, the rest shown again (not reported).  Wall clock = host time from the first setter (rebuild: from rt_scene_create) to a
context synchronise behind the update / build; device = rt_scene_update_ms / rt_scene_build_ms.  Medians and interquartile ranges over N >= 20
steps after W warm-up steps.  Measured, not gated.  --parent runs `full` and `rebuild` only, on a library without the mask calls (the parent
commit's, named by DXR_AMD_LIB)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from dxrexperiments_amd import capi, scenes  # noqa: E402
from tlas_update_timing import quartiles, turned  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent", action="store_true")
    args = ap.parse_args()
    assert args.updates >= 20, "at least 20 timed steps"
    if args.parent:                            # (a library from before the mask calls: bind what it has)
        for name in ("rt_scene_set_instance_mask", "rt_scene_set_instance_masks", "rt_scene_get_instance_masks"):
            capi.SIGNATURES.pop(name, None)
    ctx = capi.Context(0)
    sus = capi.Model(ctx, path=os.path.join(ROOT, "tests", "golden", "susanne.obj"))
    blob = capi.Model(ctx, *scenes.blob_mesh(level=3))
    xf0 = scenes.instance_grid(64)
    n = xf0.shape[0]
    models = [sus if k % 2 == 0 else blob for k in range(n)]
    scene = capi.Scene(ctx)
    for k in range(n):
        scene.add_model(models[k], xf0[k])
    scene.build()
    ctx.synchronize()
    steps = args.warmup + args.updates
    poses = [turned(xf0, s + 1) for s in range(steps)]
    moved = 2000                               # (even: visible in every case)
    half = np.where(np.arange(n) % 2 == 0, 0xFF, 0).astype(np.uint8)
    three_quarters = half.copy()
    three_quarters[1::4] = 0xFF
    everything = np.full(n, 0xFF, np.uint8)
    keys = ("full", "rebuild") if args.parent else ("full", "rebuild", "half", "quarter")
    wall = dict((k, []) for k in keys)
    dev = dict((k, []) for k in keys)

    def timed(key, s, work, ms):
        t0 = time.perf_counter()
        work()
        ctx.synchronize()
        t1 = time.perf_counter()
        if s >= args.warmup:
            wall[key].append((t1 - t0) * 1e3)
            dev[key].append(ms())

    keep = [None]
    for s in range(steps):
        xf = poses[s]

        def full():
            scene.set_transform(moved, xf[moved])
            scene.update()
        timed("full", s, full, scene.update_ms)

        def rebuild():
            sc = capi.Scene(ctx)
            for k in range(0, n, 2):
                sc.add_model(models[k], xf[k] if k == moved else xf0[k])
            sc.build()
            if keep[0] is not None:
                keep[0].close()
            keep[0] = sc
        timed("rebuild", s, rebuild, lambda: keep[0].build_ms())
        if args.parent:
            continue

        def hide_half():
            scene.set_masks(0, half)
            scene.set_transform(moved, xf0[moved])
            scene.update()
        timed("half", s, hide_half, scene.update_ms)

        def show_quarter():
            scene.set_masks(0, three_quarters)
            scene.update()
        timed("quarter", s, show_quarter, scene.update_ms)
        scene.set_masks(0, everything)
        scene.update()
        ctx.synchronize()
    print("scene: scenes.instance_grid(64), %d instances of susanne.obj and blob_mesh(level=3); %d timed steps after %d warm-up steps%s"
          % (n, args.updates, args.warmup, "; the parent's library" if args.parent else ""))
    print("%-64s %10s %10s %12s" % ("", "wall ms", "wall IQR", "device ms"))
    labels = {"full": "update, nothing hidden, 1 transform pending",
              "rebuild": "hide by a second scene: 2048 x add_model + rt_scene_build",
              "half": "masked update: 2048 hidden + 1 transform pending",
              "quarter": "masked update: 1024 of them shown again"}
    for key in keys:
        med, iqr = quartiles(wall[key])
        dmed, _ = quartiles(dev[key])
        print("%-64s %10.3f %10.3f %12.3f" % (labels[key], med, iqr, dmed))
    return 0


if __name__ == "__main__":
    sys.exit(main())
