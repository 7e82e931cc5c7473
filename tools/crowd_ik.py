#!/usr/bin/env python3
"""What solving a crowd's reaches and aims costs (rt_crowd_solve_ik = one k_crowd_ik, after one upload when the values are the host's)
beside the loop it replaces: one rt_skeleton_solve_ik (k_skeleton_ik + k_skeleton_pose) per actor on as many skeletons, the code as it was
before crowds could solve.

  python3 tools/crowd_ik.py [--actors N ...] [--chains C ...] [--steps S] [--warmup W] [--repeats R] [--no-loop]

The rig is the 65-joint comb (a root, 16 limbs of three joints, 16 single joints: it takes 32 independent constraints, two-bone and aim in
turn); per actor count (default 196 and 4096) and chain count (default 2 and 32), every actor with its own targets, poles and weights:
  stream time: R frames of solving back to back between two events on the context's stream, per frame (the gaps between launches included);
  host time:   the host clock around the calls of one frame, enqueue only, per frame -- through ctypes, whose own cost per call (about a
               microsecond) is part of the loop's figure as it is of any caller's through this binding;
for rt_crowd_solve_ik with the values in device memory (a table of 16 frames uploaded once: one launch, nothing crosses), with the values
in host memory (checked, staged and uploaded every frame), and for the loop of skeletons (its constraints packed before the clock starts;
the loop runs R / 5 frames a sample, at least one).  Medians and interquartile ranges over S >= 20 samples after W warm-up samples.  For the
kernels alone, run ONE configuration under `rocprofv3 --kernel-trace --stats -- python3 tools/crowd_ik.py --actors N --chains C`: the trace
names k_crowd_ik, k_skeleton_ik and k_skeleton_pose.  Nothing here gates: the figures are recorded."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from skeleton_timing import Events  # noqa: E402
from dxrexperiments_amd import capi, rtypes as T  # noqa: E402

LIMBS = TEETH = 16


def comb():
    """(parents, inverse binds, a pose): joint 0 the root, limb l the chain 1 + 3 l, 2 + 3 l, 3 + 3 l, then 16 single joints on the root"""
    p = [-1]
    for l in range(LIMBS):
        p += [0, 1 + 3 * l, 2 + 3 * l]
    parents = np.array(p + [0] * TEETH, np.int32)
    n = len(parents)
    rng = np.random.default_rng(1)
    ib = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (n, 1))
    ib[:, [3, 7, 11]] = rng.uniform(-1, 1, (n, 3))
    pose = np.zeros((n, 10), np.float32)
    pose[:, 0:3] = rng.uniform(-0.5, 0.5, (n, 3)) + np.array([0, 0.75, 0])
    q = rng.normal(size=(n, 4))
    pose[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    pose[:, 7:10] = 1.0
    return parents, ib, pose


def chains(n):
    """n independent chains: two-bone on a limb's last joint and aim on a single joint, in turn"""
    out = np.zeros(n, T.SKELETON_IK)
    for k in range(n):
        out[k] = (T.IK_TWO_BONE, 3 + 3 * (k // 2), (0, 0, 0), (0, 0, 2), 1.0) if k % 2 == 0 else (T.IK_AIM, 1 + 3 * LIMBS + k // 2, (0, 0, 0), (0, 1, 0), 1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", type=int, nargs="+", default=[196, 4096])
    ap.add_argument("--chains", type=int, nargs="+", default=[2, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed samples"
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
        print("%-96s stream %9.1f us (IQR %.1f)   host %9.1f us (IQR %.1f) per frame" % (label, sm, s3 - s1, hm, h3 - h1), flush=True)

    for n_actors in args.actors:
        shared = capi.Skeleton(ctx, parents, ib)
        crowd = capi.Crowd(shared, n_actors)
        crowd.set_poses(np.tile(pose, (n_actors, 1, 1)))
        singles = [capi.Skeleton(ctx, parents, ib) for _ in range(0 if args.no_loop else n_actors)]
        for sk in singles:
            sk.set_pose(pose)
        handles = [sk.h for sk in singles]
        for n_chains in args.chains:
            rng = np.random.default_rng(n_actors + n_chains)
            targets = rng.uniform(-2, 2, (frames, n_actors, n_chains, 3)).astype(np.float32)
            poles = rng.uniform(-2, 2, (frames, n_actors, n_chains, 3)).astype(np.float32)
            weights = rng.uniform(0.25, 1.0, (frames, n_actors, n_chains)).astype(np.float32)
            list_ = chains(n_chains)
            crowd.set_ik_chains(list_)
            tables = [ctx.upload(x) for x in (targets, poles, weights)]
            solve = lib.rt_crowd_solve_ik
            handle = crowd.h
            strides = [4 * n_actors * n_chains * k for k in (3, 3, 1)]
            bases = [t.ptr for t in tables]

            def device_frame(f):
                solve(handle, bases[0] + (f % frames) * strides[0], bases[1] + (f % frames) * strides[1], bases[2] + (f % frames) * strides[2], capi.MEM_DEVICE)

            host_ptrs = [[x[f].ctypes.data_as(C.c_void_p) for f in range(frames)] for x in (targets, poles, weights)]

            def host_frame(f):
                solve(handle, host_ptrs[0][f % frames], host_ptrs[1][f % frames], host_ptrs[2][f % frames], capi.MEM_HOST)

            head = "%4d actors x %d joints, %2d chains: " % (n_actors, n, n_chains)
            report(head + "rt_crowd_solve_ik, values on the device (one launch)", timed(device_frame, args.repeats))
            report(head + "rt_crowd_solve_ik, values on the host (checked, one upload, one launch)", timed(host_frame, args.repeats))
            if not args.no_loop:
                # the constraints of every actor and frame, packed before the clock starts
                packed = np.zeros((frames, n_actors, n_chains), T.SKELETON_IK)
                packed["kind"], packed["joint"] = list_["kind"][None, None, :], list_["joint"][None, None, :]
                packed["target"], packed["pole"], packed["weight"] = targets, poles, weights
                ptrs = [[packed[f, a].ctypes.data_as(C.c_void_p) for a in range(n_actors)] for f in range(frames)]
                solve_one = lib.rt_skeleton_solve_ik

                def loop_frame(f):
                    for h, p in zip(handles, ptrs[f % frames]):
                        solve_one(h, n_chains, p)

                report(head + "loop of rt_skeleton_solve_ik (2 launches an actor)", timed(loop_frame, max(1, args.repeats // 5)))
                report(head + "rt_crowd_solve_ik, values on the device, again (spread)", timed(device_frame, args.repeats))
            ctx.synchronize()
            for t in tables:
                t.close()
        ctx.synchronize()
        crowd.close()
        for sk in singles + [shared]:
            sk.close()
    ev.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
