"""The binary32 values every binary32 -> binary16 conversion of the project is held to: the oracle's round_to_half on the CPU
(test_oracle.py::test_round_to_half_is_ieee) and the device's three (k_denoise_f16, k_f32_to_f16, the RGBA16F rounding of accumulate();
test_gpu_post_chain_edges.py).  Deterministic."""
import numpy as np


def values():
    """every non-negative half, every midpoint between two neighbouring halves (a tie) with its two fp32 neighbours, the negatives of the midpoints,
    named constants (the last half 65504, the first value that rounds to infinity 65520, half of the smallest half subnormal and its neighbours, the
    infinities), random blocks at four scales; then NaN, fp32 subnormals, +-65504, +-65520 and the fp32 values next to +-65520"""
    f = np.float32
    r = np.random.default_rng(1)
    h = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)
    mid = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32)
    x = np.concatenate([r.uniform(-70000, 70000, 100000), r.normal(size=100000) * 1e-5, r.normal(size=100000) * 1e-7, r.normal(size=100000),
                        [0, -0.0, 65504, 65519.99, 65520, 1e9, 5.96e-8, 2.98e-8, 2.9802322e-8, 3e-8, np.inf, -np.inf]]).astype(np.float32)
    x = np.concatenate([x, h, mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)), -mid])
    sub = np.concatenate([[1, 2, 0x400000, 0x7FFFFF], r.integers(1, 0x800000, 60)]).astype(np.uint32).view(np.float32)      # fp32 subnormals
    top = np.array([65504, 65520, np.nextafter(f(65520), f(0)), np.nextafter(f(65520), f(np.inf))], np.float32)
    return np.concatenate([x, [f(np.nan)], sub, -sub, top, -top]).astype(np.float32)


def image(width=641):
    """values() in the RGB channels of a float32[H, W, 4] image of odd width and height (no multiple of any block size: the element-wise kernels
    meet a partial last block), alpha 1, the unused tail 0"""
    v = values()
    pixels = -(-v.size // 3)
    height = -(-pixels // width) | 1
    assert width % 2 == 1 and (width * height) % 256 != 0
    rgb = np.zeros(width * height * 3, np.float32)
    rgb[:v.size] = v
    img = np.ones((height, width, 4), np.float32)
    img[..., :3] = rgb.reshape(height, width, 3)
    return img
