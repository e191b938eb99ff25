"""Line-of-sight optical depths on the device, measured on bench.py's cfg2 frame (1e6 resident photons, the whole 1 048 576-cell frame staged):
    python tools/sightline_bench.py [--reps 5] [--photons 1000000] [--nzc 64] [--only NAME] [--no-host]
    python tools/sightline_bench.py --kernels          kernel times of sightline_kernel and of lookup_kernel on the same midpoints
Workloads (NAME): cfg2 -- step_frac 0.01, max_steps 1024, the benchmark's jet; dense -- the same mesh with the jet at lumi 1e54 (a hundred times the
optical depth) and step_frac 1e-4, some 300 steps across the mesh: the ray lengths are most ragged with tau_stop = 20.  Each with tau_stop = +inf and
20, in the plain form and with lane refill (MCRAT_HIP_SIGHTLINE_REFILL), five repeats.
Times: a host clock around mcrat_hip_sightline_photons with every output pointer NULL -- a 64-byte memset, the kernel, a 40-byte copy, the
synchronise -- so that it is the kernel's time to some tens of microseconds; and around the call with every plane read back.  Prints steps per
second and the gathered bytes per second, counted as 16 B of BucketDir + 128 B of FatCell per step.  The two forms must agree bit for bit.
Beside the call: the read-back route -- mcrat_hip_get_hydro + mcrat_hip_get_photons_soa + the NumPy checker of the tests on a subsample of rays, scaled
to the list -- whose tau must agree with the device's to the checker's bound.
--kernels takes no times itself: it starts a fresh process of this script per workload (plain form, tau_stop = +inf) under rocprofv3 with a kernel
trace and statistics; that process also hands the midpoints of its first 65 536 rays, step by step in ray order -- the order in which the march
gathers them -- to mcrat_hip_lookup_cell, whose lookup_kernel does the same two dependent gathers with none of the march's arithmetic: the floor."""
import argparse
import csv
import ctypes as C
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcrat_amd import engine, synth  # noqa: E402

GATHER_BYTES = 16 + 128
WORKLOADS = {"cfg2": dict(lumi=3e50, step_frac=0.01), "dense": dict(lumi=1e54, step_frac=1e-4)}
H_MIN, MAX_STEPS = 1e6, 1024
FLOOR_RAYS = 65536


def raw_call(e, hydro, par):
    """mcrat_hip_sightline_photons with no plane read back -> n_status"""
    out = engine.Sightlines()
    e._check(e.lib.mcrat_hip_sightline_photons(e.ctx, hydro.ctx, C.byref(par), C.byref(out)), "sightline_photons")
    return np.array(list(out.n_status), dtype=np.int64)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def fmt(ts):
    return "median %9.3f ms  (min %9.3f, max %9.3f, %d calls)" % (statistics.median(ts), min(ts), max(ts), len(ts))


def midpoints(ph, steps, step_frac, m):
    """hydro coordinates (2-D cylindrical) of the midpoints of the first m rays, step-major, with the definition's expressions"""
    p1, p2, p3 = (ph[k][:m] for k in ("p1", "p2", "p3"))
    ipn = 1 / np.sqrt((p1 * p1 + p2 * p2) + p3 * p3)
    d = (p1 * ipn, p2 * ipn, p3 * ipn)
    x, y, z = (ph[k][:m].copy() for k in ("r0", "r1", "r2"))
    a0, a1 = [], []
    for k in range(int(steps[:m].max())):
        act = steps[:m] > k
        rho = np.sqrt((x * x + y * y) + z * z)
        h = step_frac * rho
        h = np.where(h > H_MIN, h, H_MIN)
        mx, my, mz = x + (0.5 * h) * d[0], y + (0.5 * h) * d[1], z + (0.5 * h) * d[2]
        a0.append(np.sqrt(mx * mx + my * my)[act])
        a1.append(mz[act])
        x, y, z = x + h * d[0], y + h * d[1], z + h * d[2]
    return np.concatenate(a0), np.concatenate(a1)


def host_route(own, whole, params, sample):
    """what a user does without the entry point: the frame and the photons back to the host, then the march in NumPy (the tests' checker, cells by
    brute force) on `sample` rays -> seconds for the read-back, seconds for the march, the checker's answer"""
    sys.path.insert(0, ROOT)
    from tests import sightline_checker as sc
    t0 = time.perf_counter()
    cols = whole.get_hydro()
    ph = own.get_photons()
    t1 = time.perf_counter()
    frame = dict(whole.frame_meta, **{k: cols[k] for k in ("r0", "r1", "r0_size", "r1_size", "v0", "v1", "gamma", "dens_lab", "temp")})
    frame["num_elements"] = cols["num_elements"]
    live = np.nonzero((ph["weight"] != 0) & (ph["type"] != b"p") & (ph["type"] != b"N"))[0][:sample]
    want = sc.march(frame, np.stack([ph[k][live] for k in ("r0", "r1", "r2")]), np.stack([ph[k][live] for k in ("p0", "p1", "p2", "p3")]), **params)
    return t1 - t0, time.perf_counter() - t1, live, want


def run(args):
    names = [args.only] if args.only else list(WORKLOADS)
    for name in names:
        w = WORKLOADS[name]
        frame, ph, cfg = synth.config2(n_photons=args.photons, nzc=args.nzc, lumi=w["lumi"])
        # the photons' own context holds their slab only (what a run stages); a second context holds the whole frame
        own = engine.Engine(cfg["dimensions"], cfg["geometry"], 0)
        r = np.sqrt(frame["r0"] ** 2 + frame["r1"] ** 2)
        own.set_hydro(synth.select_slab(frame, np.abs(r - 1e12) < 3 * synth.C_LIGHT / 5.0))
        own.set_photons(ph)
        whole = engine.Engine(cfg["dimensions"], cfg["geometry"], 0)
        whole.set_hydro(frame)
        whole.frame_meta = {k: frame[k] for k in ("dimensions", "geometry", "r0_domain", "r1_domain", "r2_domain")}
        n = own.n
        print("== %s: %d photons, %d cells, step_frac %g, h_min %g, max_steps %d" % (name, n, frame["num_elements"], w["step_frac"], H_MIN, MAX_STEPS), flush=True)
        for tau_stop in (np.inf, 20.0):
            if args.kernels_child and tau_stop != np.inf:
                continue
            par = engine.SightlineParams(w["step_frac"], H_MIN, MAX_STEPS, tau_stop, -1.0)
            results = {}
            for refill in ("0", "1"):
                if args.kernels_child and refill == "1":
                    continue
                os.environ["MCRAT_HIP_SIGHTLINE_REFILL"] = refill
                ts = timed(lambda: raw_call(own, whole, par), args.reps)
                res = own.sightline_photons(w["step_frac"], H_MIN, MAX_STEPS, tau_stop, hydro=whole)
                tf = timed(lambda: own.sightline_photons(w["step_frac"], H_MIN, MAX_STEPS, tau_stop, hydro=whole), max(2, args.reps // 2), warm=1)
                results[refill] = res
                total = int(res["steps"].sum())
                med = statistics.median(ts) * 1e-3
                print("  tau_stop %-4g refill %s  kernel-only call %s   with read-back %s" % (tau_stop, refill, fmt(ts), fmt(tf)))
                print("      steps %d (mean %.1f, max %d per marched ray), status %s: %.3g steps/s, %.1f GB/s gathered" %
                      (total, total / max(1, int((res["status"] > 0).sum())), int(res["steps"].max()), res["n_status"].tolist(), total / med,
                       total * GATHER_BYTES / med / 1e9), flush=True)
            if len(results) == 2:
                for k in results["0"]:
                    a, b = results["0"][k], results["1"][k]
                    same = np.array_equal(a.view(np.int64), b.view(np.int64)) if a.dtype == np.float64 else np.array_equal(a, b)
                    assert same, "the two forms differ in " + k
                print("  tau_stop %-4g the two forms agree bit for bit in every output" % tau_stop)
            os.environ.pop("MCRAT_HIP_SIGHTLINE_REFILL", None)
            if tau_stop == np.inf and (args.kernels_child or not args.no_host):
                # the lookup floor's input: the same midpoints in the same order
                res = results["0"]
                m = min(FLOOR_RAYS, n)
                a0, a1 = midpoints(ph, res["steps"], w["step_frac"], m)
                sub = dict(r=[ph[k][:m] for k in ("r0", "r1", "r2")], p=[ph[k][:m] for k in ("p0", "p1", "p2", "p3")])
                ts = timed(lambda: own.sightline_rays(sub["r"], sub["p"], w["step_frac"], H_MIN, MAX_STEPS, tau_stop, hydro=whole), 3, warm=1)
                t0 = time.perf_counter()
                cells = whole.lookup_cell(a0, a1)
                print("  floor: %d midpoints of the first %d rays; mcrat_hip_lookup_cell as a call (allocations and copies included) %.1f ms, every midpoint in a cell: %s;"
                      " sightline_rays on those rays %s" % (len(a0), m, (time.perf_counter() - t0) * 1e3, bool((cells >= 0).all()), fmt(ts)))
                print("floor_steps=%d" % len(a0), flush=True)
            if tau_stop == np.inf and name == "cfg2" and not args.no_host and not args.kernels_child:      # (the dense workload's ~300 steps per ray: minutes of NumPy)
                t_back, t_march, live, want = host_route(own, whole, dict(step_frac=w["step_frac"], h_min=H_MIN, max_steps=MAX_STEPS), args.host_sample)
                res = results["0"]
                err = np.abs(res["tau"][live] - want["tau"])
                ok = ~want["fragile"]
                assert np.array_equal(res["steps"][live][ok], want["steps"][ok]) and (err[ok] <= want["bound"][ok]).all(), "device and checker disagree"
                print("  read-back route: get_hydro + get_photons_soa %.1f ms; the NumPy march of %d rays %.2f s -> %.3g s for the list; tau agrees within the bound"
                      % (t_back * 1e3, len(live), t_march, t_march * n / max(1, len(live))), flush=True)
        own.close()
        whole.close()


def kernel_rows(d):
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            for key in ("sightline_kernel", "lookup_kernel"):
                if key in row["Name"]:
                    rows.setdefault(key, []).append((int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3))
    return rows


def kernels(args):
    for name in ([args.only] if args.only else list(WORKLOADS)):
        d = tempfile.mkdtemp(prefix="sightline_%s_" % name)
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--kernels-child", "--only", name, "--reps", str(args.reps), "--photons", str(args.photons), "--nzc", str(args.nzc)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            sys.exit("%s\n%s\nexit %d: %s" % (r.stdout[-2000:], r.stderr[-2000:], r.returncode, " ".join(cmd)))
        print(r.stdout)
        for key, rows in kernel_rows(d).items():
            for calls, avg, lo, hi in rows:
                print("  %-18s calls %3d  avg %10.1f us  min %10.1f  max %10.1f" % (key, calls, avg, lo, hi))
        print("  (sightline_kernel: the calls on the whole list and, fewer, on the first %d rays are separate instantiations -- photon columns, caller rays;"
              " lookup_kernel ran once on floor_steps midpoints)" % FLOOR_RAYS, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--photons", type=int, default=1_000_000)
    ap.add_argument("--nzc", type=int, default=64)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-sample", type=int, default=16)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels:
        kernels(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
