#!/usr/bin/env python3
"""What solving IK constraints on the device costs (rt_skeleton_solve_ik = k_skeleton_ik + k_skeleton_pose) beside the host round trip it
replaces (rt_skeleton_read_pose, which synchronises, + rt_skeleton_set_pose(RT_MEM_HOST), which uploads and synchronises again; the host's
own solve is not counted: the figure is the floor of that path).

  python3 tools/skeleton_ik_timing.py [--joints N ...] [--constraints C ...] [--steps S] [--warmup W] [--repeats R]

Per joint count (default 64 and 1025: the pose behind the solve from LDS and from global memory) a comb -- a root, 15 limbs of three joints
and single joints for the rest, all under the root -- that takes 32 independent constraints: a two-bone reach on each limb, aims on the
single joints.  Per constraint count (default 1, 4 and 32): R back-to-back calls between two events on the context's stream, per call; the
figures include the gaps between back-to-back launches.  Medians and interquartile ranges over S >= 20 samples after W warm-up samples.  For
the kernel alone, run ONE joint count and ONE constraint count under `rocprofv3 --kernel-trace --stats -- python3
tools/skeleton_ik_timing.py --joints N --constraints C`: the trace names k_skeleton_ik and k_skeleton_pose.  Nothing here gates: the
figures are recorded."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from skeleton_timing import Events  # noqa: E402
from dxrexperiments_amd import capi, rtypes as T  # noqa: E402

LIMBS = 15


def comb(n):
    """(parents, pose, the 32 constraints) of a comb of n >= 64 joints"""
    assert n >= 64
    parents = [-1]
    for l in range(LIMBS):
        parents += [0, 1 + 3 * l, 2 + 3 * l]
    parents += [0] * (n - len(parents))
    rng = np.random.default_rng(n)
    pose = np.zeros((n, 10), np.float32)
    pose[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    q = rng.normal(size=(n, 4))
    pose[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    pose[:, 7:10] = 1.0
    constraints, aims = [], 0
    for k in range(T.SKELETON_MAX_IK):
        two = k % 2 == 0 and k // 2 < LIMBS
        joint = 3 + 3 * (k // 2) if two else 1 + 3 * LIMBS + aims
        aims += not two
        constraints.append(("two_bone" if two else "aim", joint, rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3), 1.0))
    return np.array(parents, np.int32), pose, constraints


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--joints", type=int, nargs="+", default=[64, 1025])
    ap.add_argument("--constraints", type=int, nargs="+", default=[1, 4, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=100)
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed samples"
    ctx = capi.Context(0)
    ev = Events(ctx)
    for n in args.joints:
        parents, pose, constraints = comb(n)
        ib = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (n, 1))
        sk = capi.Skeleton(ctx, parents, ib)
        sk.set_pose(pose)

        def timed(call):
            out = []
            for s in range(args.warmup + args.steps):
                ctx.synchronize()
                ev.record(0)
                for r in range(args.repeats):
                    call(r)
                ev.record(1)
                ms = ev.ms() / args.repeats
                if s >= args.warmup:
                    out.append(ms * 1e3)
            q1, med, q3 = np.percentile(out, [25, 50, 75])
            return med, q3 - q1
        rows = []
        for count in args.constraints:
            records = capi.Skeleton.constraints(constraints[:count])

            def solve(r, records=records):
                records["target"][:, 0] = 0.01 * (r % 50)
                sk.solve_ik(records)
            rows.append(("rt_skeleton_solve_ik, %2d constraints (k_skeleton_ik + k_skeleton_pose)" % count, solve))
        rows.append(("rt_skeleton_read_pose + rt_skeleton_set_pose(RT_MEM_HOST): the round trip a host solve takes", lambda r: sk.set_pose(sk.pose())))
        for label, call in rows:
            med, iqr = timed(call)
            print("%5d joints: %-100s %8.2f us per call (IQR %.2f), %d back-to-back calls per sample" % (n, label, med, iqr, args.repeats))
        ctx.synchronize()
        sk.close()
    ev.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
