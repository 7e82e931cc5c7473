#!/usr/bin/env python3
"""The primary stage's entry lists on the bench view (run on the GPU box): for the walk from the root and for every cut given, the primary
stage's time per frame in sets of 32 frames and frame by frame, what count_walk tallies for the primary rays (node steps per ray, from
global memory and from the LDS top; triangle tests per ray), and the lists themselves (entries per tile: mean and maximum, the share
of tiles that fell back to a coarser cut).
usage: tools/primary_entries_stats.py [cut ...]        (default: 128)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
from dxrexperiments_amd import capi, rtypes as T, scenes

W, H, S = 1920, 1080, 32
EMPTY = 0x7FFFFFFE
cuts = [int(a) for a in sys.argv[1:]] or [128]
v, t = scenes.sponza_class(seed=42)
c = scenes.sponza_camera()
cam = capi.camera_array(c["eye"], c["at"], c["up"], c["fov"], W / H)
for cut in [None] + cuts:
    ctx = capi.Context(0)
    if cut is None:
        ctx.set_option("primary_entries", 0)
    else:
        ctx.set_option("primary_entries_cut", cut)
    sc = capi.Scene(ctx); sc.add_model(capi.Model(ctx, v, t))
    p = capi.Pipeline(ctx); p.set_scene(sc)
    p.add_material(T.default_material()); p.set_environment_cube(scenes.sky_cubemap(64)); p.create_output(W, H); p.build_acceleration_structures()
    host = capi.ProgressiveHost(1234)
    f = 0
    ms = {}
    for form, per_set, sets in (("sets", S, 6), ("frames", 1, 40)):
        for timed in (False, True):
            if timed:
                p.enable_timing(64); p.reset_totals()
            for _ in range(sets if timed else 2):
                pfcs = []
                for _ in range(per_set):
                    f += 1
                    pfcs.append(host.update(cam, 0.0, f, W, H))
                if per_set > 1:
                    p.render_batch(pfcs)
                else:
                    p.update(pfcs[0]); p.render()
        tot = p.totals()
        ms[form] = (tot["ms_primary"] / tot["frames"], tot["ms_total"] / tot["frames"])
        p.enable_timing(0)
    p.render_batch([host.update(cam, 0.0, f + 1 + k, W, H) for k in range(4)])
    w = p.count_walk()["primary"]
    rays = max(w["rays"], 1)
    line = "%-9s primary %.4f of %.4f ms/frame in sets, %.4f of %.4f frame by frame | per ray: node steps %.2f (global %.2f, LDS %.2f), triangle tests %.2f" % (
        "root" if cut is None else "cut %d" % cut, ms["sets"][0], ms["sets"][1], ms["frames"][0], ms["frames"][1],
        (w["nodes_global"] + w["nodes_lds"]) / rays, w["nodes_global"] / rays, w["nodes_lds"] / rays, w["tris"] / rays)
    codes, tnear, used_cut = p.primary_entries()
    if codes is not None:
        n = (codes != EMPTY).argmin(axis=1)
        live = np.arange(codes.shape[1])[None, :] < n[:, None]
        fell = (live & (codes >= 0) & (codes < used_cut)).any(axis=1)
        line += " | lists: %d tiles, %.2f entries on average, %d at most, %.2f %% of the tiles on a coarser cut, %.2f %% empty" % (
            codes.shape[0], n.mean(), n.max(), 100.0 * fell.mean(), 100.0 * (n == 0).mean())
    print(line, flush=True)
    p.close(); sc.close(); ctx.close()
