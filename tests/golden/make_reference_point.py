"""Writes tests/golden/reference_point/<key>.npz: inputs and the results of the reference's compiled point physics
(oracle/_ref/libtpsref_point.so) for the configurations of ref_point_lib.FIXTURE_KEYS, 64 states each.  Needs a
checkout of the reference.  tests/test_reference_point.py::test_fixtures_regenerate_bit_for_bit keeps them honest;
tests/test_gpu_reference_point.py reads them where neither the library nor the checkout exists.

    python tests/golden/make_reference_point.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import ref_point_lib as R  # noqa: E402

if __name__ == "__main__":
    os.makedirs(R.FIXTURE_DIR, exist_ok=True)
    total = 0
    for key in R.FIXTURE_KEYS:
        np.savez_compressed(R.fixture_path(key), **R.fixture_arrays(key))
        size = os.path.getsize(R.fixture_path(key))
        total += size
        assert size < 200_000, (key, size)
        print(f"{key}: {size} bytes")
    assert total < 1_000_000
