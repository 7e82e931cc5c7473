"""Authoring script for tests/golden/reference_assets/: the reference checkout's own asset files, stored so that the tests that
pin them (tests/test_reference_assets.py, tests/test_sanitized_parsers.py) run from this repository alone.

    python tests/golden/make_reference_copies.py PATH_OF_THE_REFERENCE_CHECKOUT

  models/cornell.obj, susanne.obj, ground.fbx   -> copied byte for byte
  textures/CathedralIrradiance.dds (768 KB)     -> CathedralIrradiance.dds.xz, the whole file
  textures/CathedralRadiance.dds (4 MB)         -> CathedralRadiance.mip0.xz: the 148-byte header and level 0 of the six faces, the
                                                   part of the file the readers return (util.radiance_map_file() rebuilds the rest)
The level-0 texels are RGBA16F with alpha 1.0 everywhere: R, G and B are stored as planes [3][6][256][256] of half-float bit
patterns, each row delta-coded (x minus x-1, mod 2^16), the low bytes of all values then the high bytes, xz-compressed."""
import lzma
import os
import shutil
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_assets")
HEADER_BYTES = 148                       # "DDS " + DDS_HEADER (124) + DDS_HEADER_DXT10 (20)


def encode_level0(dds_bytes):
    size, mips = struct.unpack_from("<I", dds_bytes, 12)[0], struct.unpack_from("<I", dds_bytes, 28)[0]
    per_face = sum((size >> m) ** 2 * 4 for m in range(mips))
    texels = np.frombuffer(dds_bytes, np.uint16, offset=HEADER_BYTES).reshape(6, per_face)[:, :size * size * 4].reshape(6, size, size, 4)
    assert (texels[..., 3] == 0x3C00).all(), "alpha is not 1.0 everywhere"
    planes = np.moveaxis(texels[..., :3], 3, 0).astype(np.int32)
    delta = np.diff(planes, axis=-1, prepend=0).astype(np.uint16)
    shuffled = np.ascontiguousarray(delta).view(np.uint8).reshape(-1, 2).T.tobytes()
    return lzma.compress(dds_bytes[:HEADER_BYTES] + shuffled, preset=9 | lzma.PRESET_EXTREME)


def main(ref):
    os.makedirs(OUT, exist_ok=True)
    for name in ("cornell.obj", "susanne.obj", "ground.fbx"):
        shutil.copyfile(os.path.join(ref, "assets", "models", name), os.path.join(OUT, name))
    with open(os.path.join(ref, "assets", "textures", "CathedralIrradiance.dds"), "rb") as f:
        irr = f.read()
    with open(os.path.join(OUT, "CathedralIrradiance.dds.xz"), "wb") as f:
        f.write(lzma.compress(irr, preset=9 | lzma.PRESET_EXTREME))
    with open(os.path.join(ref, "assets", "textures", "CathedralRadiance.dds"), "rb") as f:
        rad = f.read()
    with open(os.path.join(OUT, "CathedralRadiance.mip0.xz"), "wb") as f:
        f.write(encode_level0(rad))
    for name in sorted(os.listdir(OUT)):
        print("%-28s %8d bytes" % (name, os.path.getsize(os.path.join(OUT, name))))


if __name__ == "__main__":
    main(sys.argv[1])
