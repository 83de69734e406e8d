"""Child of tests/test_gpu_match_edges.py::test_kernel_variant: the matcher reads VX_MATCH_SHAPE, VX_MATCH_CHUNKED
and VX_MATCH_GRID once per process, so every variant runs in a fresh process with the variable in its environment.

    python match_variant_child.py cases.npz results.npz

cases.npz holds n, and per case i: q_i, t_i (uint8 rows of 32) and ratio_i; results.npz gets m_i, the matches of
Context.match(q_i, t_i, ratio_i).  Imports numpy and vxslam only.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visionx-slam_amd", "python"))

import vxslam  # noqa: E402


def main(src, dst):
    cases = np.load(src)
    ctx = vxslam.Context(0)
    out = {}
    try:
        for i in range(int(cases["n"])):
            out[f"m_{i}"] = ctx.match(cases[f"q_{i}"], cases[f"t_{i}"], float(cases[f"ratio_{i}"]))
    finally:
        ctx.close()
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
