#!/usr/bin/env python3
"""What an ordered list of IK groups costs in one call (rt_crowd_solve_ik over a list of rt_crowd_set_ik_chain_groups = one k_ik_groups;
rt_skeleton_solve_ik_groups = one k_ik_groups with one block) beside the only way there was before groups: per group one
rt_crowd_set_ik_chains plus one rt_crowd_solve_ik on that group's own slices of the value arrays (one k_crowd_ik a group), and for the
single skeleton one rt_skeleton_solve_ik per group (k_skeleton_ik + k_skeleton_pose a group).

  python3 tools/ik_groups.py [--actors N ...] [--groups G ...] [--steps S] [--warmup W] [--repeats R]

The rig is the 65-joint comb (a root, 16 limbs of three joints, 16 single joints); per actor count (default 196 and 4096) and group count
(default 1, 2, 4 and 8) a list of 32 constraints: with one group the 32 independent ones of tools/crowd_ik.py; with G > 1 groups a reach on
every limb in the first G / 2 groups and an aim of every limb's tip in the last G / 2, so that every aim depends on a reach.  Every actor
has its own targets, poles and weights, in device memory (a table of 16 frames uploaded once, whole for the grouped call and sliced by group
for the other way):
  stream time: R frames of solving back to back between two events on the context's stream, per frame (the gaps between launches included);
  host time:   the host clock around the calls of one frame, enqueue only, per frame -- through ctypes, whose own cost per call (about a
               microsecond) is part of every figure.
Medians and interquartile ranges over S >= 20 samples after W warm-up samples.  Nothing here gates: the figures are recorded (DESIGN.md
section 7)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crowd_ik import LIMBS, chains, comb  # noqa: E402
from skeleton_timing import Events  # noqa: E402
from dxrexperiments_amd import capi, rtypes as T  # noqa: E402


def grouped_list(n_groups):
    """(sizes, rtypes.SKELETON_IK[32]): one group of 32 independent constraints, or reaches then aims of their tips in n_groups groups"""
    if n_groups == 1:
        return [32], chains(32)
    out = np.zeros(2 * LIMBS, T.SKELETON_IK)
    for l in range(LIMBS):
        out[l] = (T.IK_TWO_BONE, 3 + 3 * l, (0, 0, 0), (0, 0, 2), 1.0)
        out[LIMBS + l] = (T.IK_AIM, 3 + 3 * l, (0, 0, 0), (0, 1, 0), 1.0)
    return [2 * LIMBS // n_groups] * n_groups, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", type=int, nargs="+", default=[196, 4096])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed samples"
    assert all(g in (1, 2, 4, 8) for g in args.groups)
    ctx = capi.Context(0)
    ev = Events(ctx)
    lib = capi.lib()
    parents, ib, pose = comb()
    n = len(parents)
    frames = 16

    def timed(frame, repeats):
        stream, host = [], []
        for s in range(args.warmup + args.steps):
            ctx.synchronize()
            ev.record(0)
            t0 = time.perf_counter()
            for r in range(repeats):
                frame(s * repeats + r)
            t1 = time.perf_counter()
            ev.record(1)
            ms = ev.ms() / repeats
            if s >= args.warmup:
                stream.append(ms * 1e3)
                host.append((t1 - t0) * 1e6 / repeats)
        return tuple(np.percentile(x, [50, 25, 75]) for x in (stream, host))

    def report(label, got):
        (sm, s1, s3), (hm, h1, h3) = got
        print("%-100s stream %9.1f us (IQR %.1f)   host %9.1f us (IQR %.1f) per frame" % (label, sm, s3 - s1, hm, h3 - h1), flush=True)

    # ---- the single skeleton ----
    single = capi.Skeleton(ctx, parents, ib)
    single.set_pose(pose)
    rng = np.random.default_rng(7)
    for n_groups in args.groups:
        sizes, list_ = grouped_list(n_groups)
        packed = np.tile(list_, (frames, 1))
        packed["target"] = rng.uniform(-2, 2, (frames, 32, 3)).astype(np.float32)
        packed["pole"] = rng.uniform(-2, 2, (frames, 32, 3)).astype(np.float32)
        packed["weight"] = rng.uniform(0.25, 1.0, (frames, 32)).astype(np.float32)
        sizes_a = np.array(sizes, np.uint32)
        ps = sizes_a.ctypes.data_as(C.c_void_p)
        whole = [packed[f].ctypes.data_as(C.c_void_p) for f in range(frames)]
        firsts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        parts = [[(sizes[g], packed[f, firsts[g]:firsts[g] + sizes[g]].ctypes.data_as(C.c_void_p)) for g in range(n_groups)] for f in range(frames)]
        h, grouped, one = single.h, lib.rt_skeleton_solve_ik_groups, lib.rt_skeleton_solve_ik

        def grouped_frame(f):
            grouped(h, n_groups, ps, whole[f % frames])

        def loop_frame(f):
            for size, p in parts[f % frames]:
                one(h, size, p)

        head = "   1 skeleton x %d joints, 32 constraints in %d groups: " % (n, n_groups)
        report(head + "rt_skeleton_solve_ik_groups (one launch)", timed(grouped_frame, args.repeats))
        report(head + "rt_skeleton_solve_ik per group (2 launches a group)", timed(loop_frame, args.repeats))
    single.close()

    # ---- the crowd ----
    for n_actors in args.actors:
        shared = capi.Skeleton(ctx, parents, ib)
        crowd = capi.Crowd(shared, n_actors)
        crowd.set_poses(np.tile(pose, (n_actors, 1, 1)))
        for n_groups in args.groups:
            sizes, list_ = grouped_list(n_groups)
            rng = np.random.default_rng(n_actors + n_groups)
            targets = rng.uniform(-2, 2, (frames, n_actors, 32, 3)).astype(np.float32)
            poles = rng.uniform(-2, 2, (frames, n_actors, 32, 3)).astype(np.float32)
            weights = rng.uniform(0.25, 1.0, (frames, n_actors, 32)).astype(np.float32)
            tables = [ctx.upload(x) for x in (targets, poles, weights)]
            firsts = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
            # the other way's arrays: every group's own slice, [frames][n_actors][size], made before the clock starts
            sliced = [[ctx.upload(np.ascontiguousarray(x[:, :, a:a + s])) for x in (targets, poles, weights)] for a, s in zip(firsts, sizes)]
            lists = [np.ascontiguousarray(list_[a:a + s]) for a, s in zip(firsts, sizes)]
            list_ptrs = [x.ctypes.data_as(C.c_void_p) for x in lists]
            solve, set_chains, handle = lib.rt_crowd_solve_ik, lib.rt_crowd_set_ik_chains, crowd.h
            strides = [4 * n_actors * 32 * k for k in (3, 3, 1)]
            bases = [t.ptr for t in tables]

            def grouped_frame(f):
                solve(handle, bases[0] + (f % frames) * strides[0], bases[1] + (f % frames) * strides[1], bases[2] + (f % frames) * strides[2], capi.MEM_DEVICE)

            def swapping_frame(f):
                for g, s in enumerate(sizes):
                    set_chains(handle, s, list_ptrs[g])
                    b = sliced[g]
                    solve(handle, b[0].ptr + (f % frames) * 12 * n_actors * s, b[1].ptr + (f % frames) * 12 * n_actors * s, b[2].ptr + (f % frames) * 4 * n_actors * s,
                          capi.MEM_DEVICE)

            head = "%4d actors x %d joints, 32 constraints in %d groups: " % (n_actors, n, n_groups)
            sz = np.array(sizes, np.uint32)
            assert lib.rt_crowd_set_ik_chain_groups(handle, n_groups, sz.ctypes.data_as(C.c_void_p), list_.ctypes.data_as(C.c_void_p)) == 0, lib.rt_last_error()
            report(head + "rt_crowd_solve_ik over the grouped list (one launch)", timed(grouped_frame, args.repeats))
            report(head + "rt_crowd_set_ik_chains + rt_crowd_solve_ik per group (one launch a group)", timed(swapping_frame, args.repeats))
            assert lib.rt_crowd_set_ik_chain_groups(handle, n_groups, sz.ctypes.data_as(C.c_void_p), list_.ctypes.data_as(C.c_void_p)) == 0, lib.rt_last_error()
            report(head + "rt_crowd_solve_ik over the grouped list, again (spread)", timed(grouped_frame, args.repeats))
            ctx.synchronize()
            for t in tables + [b for part in sliced for b in part]:
                t.close()
        ctx.synchronize()
        crowd.close()
        shared.close()
    ev.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
