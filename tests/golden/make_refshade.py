"""Record tests/golden/refshade/*.npz from the reference's own shading text compiled as C++ (oracle/_ref/librefshade.so; `make oracle`
builds it where the reference checkout is present).  The cases are tests/refshade_cases.py; tests/test_refshade.py regenerates them
in memory and requires equality with the committed files, so run this after any change to the cases:

    python tests/golden/make_refshade.py

Only recorded inputs and outputs are written: no reference text.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import refshade_cases as R                   # noqa: E402
from oracle import pyoracle                  # noqa: E402

MAX_BYTES = 456994                           # the largest fixture committed before these (denoise_mock.npz)


def generate():
    """name -> dict of arrays, from librefshade.so"""
    pyoracle.build()
    ref = R.Ref(pyoracle)
    out = {"units": R.compute_units(ref)}
    for name, case in R.frame_cases(pyoracle).items():
        out[name] = R.compute_frame(ref, pyoracle, case)
    return out


def main():
    os.makedirs(R.FIXTURES, exist_ok=True)
    made = generate()
    made.update(R.split_units(made.pop("units")))
    for name, arrays in made.items():
        path = R.fixture_path(name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print("%-60s %7d bytes" % (os.path.basename(path), size))
        assert size <= MAX_BYTES, "%s is larger than the largest fixture committed before" % path


if __name__ == "__main__":
    main()
