"""Diagnostic: where a virtual rank's workgroup spends a frame (s_memtime ticks, -DMCRAT_DIAG build).

Two runs per frame: the phases of a list's frame, then (mcrat_hip_diag_set(2048)) the serial stretch of a non-forced pass between phase 1 and
the event walk, stamp by stamp.  MCRAT_HIP_LIB names another diagnostic build of the same ABI (before / after)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcrat_amd import build, engine, synth  # noqa: E402

diag_lib = os.path.join(os.path.dirname(build.LIB), "libmcrat_hip_diag.so")
if not os.environ.get("MCRAT_HIP_LIB"):
    if not (os.environ.get("MCRAT_DIAG_PREBUILT") and os.path.exists(diag_lib)):     # (built here beforehand: the library travels with the snapshot)
        build.build(force=True, extra_flags=["-DMCRAT_DIAG=1"], lib=diag_lib, objdir=os.path.join(os.path.dirname(build.LIB), "_obj_diag"))
    engine.LIB_PATH = diag_lib
lib = engine.load_library()
lib.mcrat_hip_diag_rank_stamps.restype, lib.mcrat_hip_diag_rank_stamps.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
lib.mcrat_hip_diag_set.restype, lib.mcrat_hip_diag_set.argtypes = C.c_int, [C.c_int]
n = int(os.environ.get("N", "1000000"))
per = int(os.environ.get("PER", "1000"))


def frame_stamps(frame, ph, cfg, bits):
    import time
    lib.mcrat_hip_diag_set(bits)
    e = engine.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], virtual_rank_photons=per)
    e.set_hydro(frame)
    e.set_photons(ph)
    e.begin_frame(1, 0.0, 1.0 / frame["fps"])
    e.synchronize()
    t0 = time.perf_counter()
    e.run(0)
    wall = (time.perf_counter() - t0) * 1e3
    rows = []
    for r in range(e.num_virtual_ranks()):
        out = (C.c_longlong * 8)()
        lib.mcrat_hip_diag_rank_stamps(e.ctx, r, out)
        rows.append(list(out))
    e.close()
    lib.mcrat_hip_diag_set(0)
    return np.array(rows, dtype=np.float64), wall


for lumi in [float(x) for x in os.environ.get("LUMI", "3e50,1e53").split(",")]:
    frame, ph, cfg = synth.config2(n_photons=n, lumi=lumi)
    a, wall = frame_stamps(frame, ph, cfg, 0)
    print("frame wall time %.3f ms" % wall)
    a *= 0.01                                       # ticks x 0.01
    passes = a[:, 5] * 100
    print("lumi %.0e: %d ranks x %d photons, passes per rank mean %.1f" % (lumi, len(a), per, passes.mean()), flush=True)
    print("   per workgroup [ticks x 0.01], mean over ranks: load %.1f | forced pass step %.1f | other passes: step %.1f (%.2f per pass) | event %.1f (%.2f per pass) | store %.1f | total %.1f"
          % (a[:, 0].mean(), a[:, 1].mean(), a[:, 2].mean(), (a[:, 2] / np.maximum(passes - 1, 1)).mean(), a[:, 3].mean(),
             (a[:, 3] / np.maximum(passes, 1)).mean(), a[:, 4].mean(), (a[:, :5].sum(axis=1) + a[:, 6] + a[:, 7]).mean()), flush=True)
    print("   of the step time: phase 1 of thread 0's wave %.1f, barrier wait %.1f, phase 2 + minimum %.1f   (ticks x 0.01; clock ~2.1 GHz)"
          % (a[:, 6].mean(), a[:, 7].mean(), a[:, 2].mean()), flush=True)
    # the serial stretch of the non-forced passes: ticks per such pass, mean over the lists that had one
    s, _ = frame_stamps(frame, ph, cfg, 2048)
    s = s[s[:, 7] > 0]
    p = s[:, 7:8]
    names = ("top of pass (its barrier, if any)", "s_qn read + phase 2", "wave minimum + publish", "counters", "barrier behind the minima", "merge")
    print("   serial stretch, ticks per non-forced pass (%.1f such passes per list, %d lists):" % (p.mean(), len(s)), flush=True)
    for k, nme in enumerate(names):
        print("      %-36s %8.0f" % (nme, (s[:, k:k + 1] / p).mean()), flush=True)
    print("      %-36s %8.0f" % ("sum of the last five", (s[:, 1:6].sum(axis=1, keepdims=True) / p).mean()), flush=True)
