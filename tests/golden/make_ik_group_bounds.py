"""Writes tests/golden/ik_group_bounds.json: what examples/realtime_crowd_grasp.cpp prints as its two measures, computed on the CPU from the
numpy statement of a grouped solve (tests/ik_group_cases.py) over the example's own inputs.  The example makes its inputs with + - * / and
fmod alone, in fp32, so they are restated here bit for bit; the kernel equals the statement bit for bit (tests/test_gpu_ik_groups.py), so
the largest aim angle the example prints is this number, to the precision of its print, and not a bound that was measured.

    python tests/golden/make_ik_group_bounds.py [frames]
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ik_cases as IK                # noqa: E402
import ik_group_cases as G           # noqa: E402
import skeleton_cases as S           # noqa: E402

F = np.float32
JOINTS, KEYS, TIP, SIDE = 4, 3, 3, 14
ACTORS = SIDE * SIDE
SPAN, PITCH, LIFT = F(0.75), F(3.0), F(0.35)
PARENTS = np.array([-1, 0, 1, 2], np.int32)
TIMES = np.array([0.0, 1.0, 2.0], F)
TURNS = np.array([[0, 0, 0, 1], [0, 0, 0.29552021, 0.95533649], [-0.24740396, 0, 0, 0.96891242]], F)


def foot_of(a):
    return PITCH * (F(a % SIDE) - F(0.5) * F(SIDE - 1)), PITCH * (F(a // SIDE) - F(0.5) * F(SIDE - 1))


def clip_of(a):
    x, z = foot_of(a)
    keys = np.zeros((KEYS, JOINTS, 10), F)
    for k in range(KEYS):
        for j in range(JOINTS):
            keys[k, j, 0:3] = (x, F(-1.5), z) if j == 0 else (F(0.0), SPAN, F(0.0))
            keys[k, j, 3:7] = TURNS[0] if j == 0 else TURNS[k]
            keys[k, j, 7:10] = 1.0
    return keys


def values_of(a, frame):
    """(time, grasp point, target) of actor a at a frame, by the example's statements in fp32"""
    x, z = foot_of(a)
    time = np.fmod(F(0.1) * F(frame) + F(0.01) * F((a * 37) % 200), TIMES[KEYS - 1])
    phase = np.fmod(F(0.05) * F(frame) + F(0.013) * F(a), F(1.0))
    u = F(2.0) * phase - F(1.0)
    den = F(1.0) + u * u
    co = (F(-1.0) if a & 1 else F(1.0)) * ((F(1.0) - u * u) / den)
    si = (F(2.0) * u) / den
    grasp = np.array([x + F(0.7) * co, F(0.15) + F(0.3) * si, z + F(0.7) * si], F)
    target = np.array([grasp[0], grasp[1] + LIFT, grasp[2]], F)
    return F(time), grasp, target


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    ib = np.zeros((JOINTS, 12), F)
    ib[:, [0, 5, 10]] = 1.0
    worst_tip = worst_angle = 0.0
    for a in range(ACTORS):
        keys = clip_of(a)
        x, z = foot_of(a)
        pole = (float(x), 0.0, float(z + F(3.0)))
        for frame in range(1, frames + 1):
            time, grasp, target = values_of(a, frame)
            held = S.sampled(TIMES, keys, time)
            groups = [[(IK.TWO_BONE, TIP, tuple(float(v) for v in grasp), pole, 1.0)], [(IK.AIM, TIP, tuple(float(v) for v in target), (0.0, 1.0, 0.0), 1.0)]]
            _, W, _ = G.solved_and_posed(PARENTS, ib, held, groups)
            hand = W[TIP].astype(np.float64)
            tip = 0.0
            axis, to = [0.0] * 3, [0.0] * 3
            for r in range(3):
                d = hand[4 * r + 3] - float(grasp[r])
                tip += d * d
                axis[r] = hand[4 * r + 1]
                to[r] = float(target[r]) - hand[4 * r + 3]
            worst_tip = max(worst_tip, math.sqrt(tip))
            cx, cy, cz = axis[1] * to[2] - axis[2] * to[1], axis[2] * to[0] - axis[0] * to[2], axis[0] * to[1] - axis[1] * to[0]
            worst_angle = max(worst_angle, math.atan2(math.sqrt(cx * cx + cy * cy + cz * cz), axis[0] * to[0] + axis[1] * to[1] + axis[2] * to[2]))
    out = {"frames": frames, "aim_angle": worst_angle, "tip_to_target": worst_tip, "chain_length": 1.5, "actors": ACTORS,
           "made_by": "tests/golden/make_ik_group_bounds.py: the numpy statement over the inputs of examples/realtime_crowd_grasp.cpp"}
    with open(os.path.join(HERE, "ik_group_bounds.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
