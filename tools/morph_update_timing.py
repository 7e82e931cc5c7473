#!/usr/bin/env python3
"""What a morphed update costs (rt_model_set_morph_weights + rt_scene_update), against the only route to the same scene before it existed:
rt_model_set_vertices from a device array of finished vertices + rt_scene_update.

  python3 tools/morph_update_timing.py [--updates N] [--warmup W] [--repeats R]

The bench scene, scenes.sponza_class() (~262 k triangles, 141,685 vertices), one identity instance, with two sets of targets, both with normal
deltas: 8 dense targets (every vertex in every target), and 50 sparse targets of 5 % of the vertices each (a run of consecutive vertices from
a random start: a local shape).
(a) Per step, alternating (so that drift hits both alike): set_vertices from a device array of that step's finished vertices + update,
set_morph_weights from a host array + update: the same mesh is rebuilt by both.  Wall clock = host time from the first call to a context
synchronise behind the last; device ms = rt_scene_update_ms.
(b) The kernel alone, all in one process and alternating sample by sample: R back-to-back calls between two events on the context's stream of
rt_model_set_vertices from device memory (a device-to-device copy of the vertex array), rt_model_set_bones (k_skin_vertices, K = 4, 64 bones,
palette in device memory), and rt_model_set_morph_weights (weights in device memory) for the dense and the sparse targets.  The figures
include the gaps between back-to-back launches.  The expectation from the code is a kernel bound by its bytes: 48 B per vertex (the base
read, the result written) + 4 B of count per vertex + 26 B per evaluated cell (2 B target, 12 B position delta, 12 B normal delta; 14 B without
normal deltas); the GB/s column is those bytes over the median.
Medians and interquartile ranges over N >= 20 steps after W warm-up steps.  Nothing here gates: the figures are recorded."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dxrexperiments_amd import capi, rtypes as T, scenes  # noqa: E402
from skin_update_timing import Events, palette_of, quartiles, slab_skin  # noqa: E402


def dense_targets(n_verts, n_targets, seed):
    rng = np.random.default_rng(seed)
    off = (np.arange(n_targets + 1, dtype=np.uint64) * n_verts).astype(np.uint32)
    idx = np.tile(np.arange(n_verts, dtype=np.uint32), n_targets)
    return off, idx, rng.uniform(-0.05, 0.05, (len(idx), 3)).astype(np.float32), rng.uniform(-0.2, 0.2, (len(idx), 3)).astype(np.float32)


def sparse_targets(n_verts, n_targets, share, seed):
    rng = np.random.default_rng(seed)
    per = int(n_verts * share)
    starts = rng.integers(0, n_verts - per, n_targets)
    off = (np.arange(n_targets + 1, dtype=np.uint64) * per).astype(np.uint32)
    idx = np.concatenate([np.arange(s, s + per, dtype=np.uint32) for s in starts])
    return off, idx, rng.uniform(-0.05, 0.05, (len(idx), 3)).astype(np.float32), rng.uniform(-0.2, 0.2, (len(idx), 3)).astype(np.float32)


def stored_cells(n_verts, idx):
    """cells of the SELL-64 layout (rt_morph.h): 64 x the longest run of every slice"""
    count = np.bincount(idx, minlength=-(-n_verts // 64) * 64)
    return int(64 * count.reshape(-1, 64).max(axis=1).sum())


def weights_of(n_targets, step):
    return (0.5 + 0.5 * np.sin(0.37 * step + 0.9 * np.arange(n_targets))).astype(np.float32)


def updates(ctx, scene, model, rest, sets, steps, warmup):
    """(a): the two routes, alternating, for every set of targets"""
    print("%-72s %12s %12s %14s" % ("", "wall ms", "wall IQR", "update_ms"))
    for label, (off, idx, dp, dn) in sets:
        model.set_vertices(rest)
        model.set_morph_targets(off, idx, dp, dn)
        nt = len(off) - 1
        wall = {"verts_device": [], "morph": []}
        dev = {"verts_device": [], "morph": []}
        for s in range(warmup + steps):
            w = weights_of(nt, s + 1)
            model.set_morph_weights(w)                       # (untimed: the finished vertices of this step, as a device producer's output --
            dbuf = ctx.upload(model.geometry()[0])           # both routes build the same mesh)
            ctx.synchronize()
            took = {}
            t0 = time.perf_counter()
            model.set_vertices_device(dbuf.ptr, len(rest))
            scene.update()
            ctx.synchronize()
            took["verts_device"] = ((time.perf_counter() - t0) * 1e3, scene.update_ms())
            t0 = time.perf_counter()
            model.set_morph_weights(w)
            scene.update()
            ctx.synchronize()
            took["morph"] = ((time.perf_counter() - t0) * 1e3, scene.update_ms())
            dbuf.close()
            if s >= warmup:
                for k, (a, b) in took.items():
                    wall[k].append(a); dev[k].append(b)
        for key, text in (("verts_device", "set_vertices (device memory) + rt_scene_update"), ("morph", "set_morph_weights (host weights, %s) + rt_scene_update" % label)):
            med, iqr = quartiles(wall[key])
            print("%-72s %12.3f %12.3f %14.3f" % (text, med, iqr, quartiles(dev[key])[0]))
    model.clear_morph_targets()
    model.set_vertices(rest)


def kernel_alone(ctx, rest, idx_tri, sets, steps, warmup, repeats):
    """(b): the morph kernel against a device-to-device copy of the vertex array and the skin kernel, alternating"""
    ev = Events(ctx)
    nv = len(rest)
    vbuf = ctx.upload(rest)
    plain, skinned = capi.Model(ctx, rest, idx_tri), capi.Model(ctx, rest, idx_tri)
    bones, sw = slab_skin(rest, 64)
    skinned.set_skin(bones, sw, 64)
    centre = 0.5 * (rest["position"].min(axis=0) + rest["position"].max(axis=0)).astype(np.float64)
    pbuf = ctx.upload(palette_of(64, 1, centre))
    calls = [("device-to-device copy of %d vertices (%.2f MB)" % (nv, 24e-6 * nv), lambda: plain.set_vertices_device(vbuf.ptr, nv), 48 * nv),
             ("k_skin_vertices, K = 4, 64 bones (LDS)", lambda: skinned.set_bones_device(pbuf.ptr), nv * (48 + 4 * 6) + ((nv + 255) // 256) * 48 * 64)]
    held = [pbuf]
    for label, (off, idx, dp, dn) in sets:
        m = capi.Model(ctx, rest, idx_tri)
        m.set_morph_targets(off, idx, dp, dn)
        wbuf = ctx.upload(weights_of(len(off) - 1, 1))
        held += [wbuf, m]
        calls.append(("k_morph_vertices<normals>, %s" % label, (lambda m=m, wbuf=wbuf: m.set_morph_weights_device(wbuf.ptr)), nv * 52 + 26 * len(idx)))
        print("%s: %d entries (cells evaluated), %d cells stored, %.2f entries per vertex" % (label, len(idx), stored_cells(nv, idx), len(idx) / nv))
    out = [[] for _ in calls]
    for s in range(warmup + steps):
        for k, (_, call, _) in enumerate(calls):
            ctx.synchronize()
            ev.record(0)
            for _ in range(repeats):
                call()
            ev.record(1)
            us = ev.ms() / repeats * 1e3
            if s >= warmup:
                out[k].append(us)
    copy = quartiles(out[0])[0]
    for (label, _, moved), v in zip(calls, out):
        med, iqr = quartiles(v)
        print("%-72s %10.2f us (IQR %.2f): %.2f x the copy; %.0f GB/s over %.2f MB" % (label, med, iqr, med / copy, 1e-3 * moved / med, 1e-6 * moved))
    ctx.synchronize()
    for h in held:
        h.close()
    plain.close(); skinned.close()
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
    v, idx = scenes.sponza_class()
    v = np.ascontiguousarray(v, T.VERTEX)
    sets = [("8 dense targets", dense_targets(len(v), 8, 1)), ("50 sparse targets of 5 %", sparse_targets(len(v), 50, 0.05, 2))]
    model = capi.Model(ctx, v, idx)
    scene = capi.Scene(ctx)
    scene.add_model(model, None)
    scene.build()
    print("bench scene: scenes.sponza_class(), %d triangles, %d vertices, one identity instance; %d timed steps after %d" % (len(idx), len(v), args.updates, args.warmup))
    updates(ctx, scene, model, v, sets, args.updates, args.warmup)
    scene.close(); model.close()
    print("the kernel alone, %d back-to-back calls per sample, the calls alternating:" % args.repeats)
    kernel_alone(ctx, v, idx, sets, args.updates, args.warmup, args.repeats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
