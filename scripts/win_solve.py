#!/usr/bin/env python3
"""k_ba_win's phase A apart: where the time between a workgroup's rows and its solve barrier goes.

Trace variant -DVX_WIN_TRACE_SOLVE (make trace-solve): slot 1 + 3i = every wave's sums of iteration i
staged (wave 0 behind the staging barrier), slot 3 + 3i = wave 0's solve done, slot 2 + 3i = the solve
barrier.  Per iteration, medians over the workgroups and 20 runs:
previous solve barrier -> sums staged -> solve done -> solve barrier.

    VX_LIB=visionx-slam_amd/lib/libvxslam_trace_solve.so python3 scripts/win_solve.py

With --plain, for the plain trace build (make trace; slot 1 + 3i = wave 0's own rows ready): wave 0's
rows ready -> solve barrier, which is all a library without the staging barrier can show.

    VX_LIB=visionx-slam_amd/lib/libvxslam_trace.so python3 scripts/win_solve.py --plain"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visionx-slam_amd", "python"))
import vxslam  # noqa: E402
from vxslam import synth  # noqa: E402

KT_BLOCKS, KT_SLOTS = 256, 16
plain = "--plain" in sys.argv[1:]
nk, nl, ns = synth.ba_config("C3")
m = synth.make_ba_map(0x5EED0003, nk, nl)
ctx = vxslam.Context(0)
plan = ctx.ba_plan(m, vxslam.default_ba_options(window=nk, iters=5))
nb = plan.layout()["workgroups"]
print("plan", plan.info(), "persistent", plan.persistent(), f"{nb} workgroups")
runs = []
for rep in range(20):
    for _ in range(5):
        plan.run_async()
    ctx.synchronize()
    out = np.zeros(2 * KT_BLOCKS * KT_SLOTS, np.int64)
    assert vxslam.lib().vx_ktrace_read_ba(C.c_void_p(out.ctypes.data)) == 0
    tr = out.reshape(2, KT_BLOCKS, KT_SLOTS)[0][:nb].astype(np.float64) / 100.0
    if (tr[:, 0] <= 0).any():
        continue
    runs.append(tr)
T = np.stack(runs)  # [runs, workgroups, slots], us


def show(name, d):  # d: [runs, workgroups, iterations]
    A = np.median(d, 0)  # per workgroup and iteration
    print(f"{name:44s} median {np.median(A):5.2f}  p90 {np.percentile(A, 90):5.2f}  max {A.max():5.2f} us   per it (median): "
          + " ".join(f"{v:5.2f}" for v in np.median(A, 0)))


print(f"{len(runs)} traced runs")
if plain:
    show("wave 0's rows ready -> solve barrier", np.stack([T[:, :, 2 + 3 * i] - T[:, :, 1 + 3 * i] for i in range(5)], 2))
    show("solve barrier -> next solve barrier", np.stack([T[:, :, 5 + 3 * i] - T[:, :, 2 + 3 * i] for i in range(4)], 2))
else:
    show("solve barrier -> next sums staged", np.stack([T[:, :, 4 + 3 * i] - T[:, :, 2 + 3 * i] for i in range(4)], 2))
    show("sums staged -> solve done (wave 0)", np.stack([T[:, :, 3 + 3 * i] - T[:, :, 1 + 3 * i] for i in range(4)], 2))
    show("solve done -> solve barrier", np.stack([T[:, :, 2 + 3 * i] - T[:, :, 3 + 3 * i] for i in range(4)], 2))
    show("sums staged -> solve barrier", np.stack([T[:, :, 2 + 3 * i] - T[:, :, 1 + 3 * i] for i in range(5)], 2))
    show("solve barrier -> next solve barrier", np.stack([T[:, :, 5 + 3 * i] - T[:, :, 2 + 3 * i] for i in range(4)], 2))
plan.close()
ctx.close()
