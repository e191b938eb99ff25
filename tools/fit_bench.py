"""Times mcrat_hip_fit_spectra (Engine.fit_spectra) on Poisson spectra: 10^4 and 6 * 10^5 spectra of 64 and 128 bins, both models, the binding's
default search.

One process per case and step, each under its own time limit, so that a limit that is hit names its step:
  calls    a host clock around Engine.fit_spectra, which uploads count and w, fits and copies the columns back, and ends in a stream synchronise;
           one warm-up call, then --reps calls: median, min and max.  With --trace this process runs under rocprofv3 --kernel-trace --stats and
           fit_kernel's row is printed beside it: the kernel time of the same calls.
  checker  what it is measured against: the NumPy restatement of the same search (tests/fit_checker.py) on one host core, timed on --host-spectra
           spectra and scaled linearly to the case's number of spectra -- an extrapolation, printed as such --, and the device's columns for those
           spectra compared with it by their bytes.  Done for the smallest size only.  No other fitter is installed beside this project, so none
           is timed.
The kernel's time is proportional to the number of spectra once the device is full, so a case of a larger size is started only if the same bins
and model at the size before predict that it stays below half its limit; otherwise a SKIPPED line says what was predicted.  Nothing more is
started after a process that failed.  Needs nothing outside the repository."""
import argparse
import csv
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fit_checker as F  # noqa: E402  (NumPy only: the shapes of the synthetic spectra, and the search that is timed beside the device)
KEV = F.KEV
SEED = 20261021


def spectra(model, n_spec, n_e, total=2e4):
    """Poisson spectra of 256 random shapes, repeated with fresh noise: 10 keV .. 10 MeV, about `total` photons each"""
    rng = np.random.default_rng(SEED + n_e + model)
    edges = np.logspace(1.0, 4.0, n_e + 1) * KEV
    cen = np.sqrt(edges[:-1] * edges[1:])
    shapes = np.array([F.band_shape(rng.uniform(-1.5, 0.3), rng.uniform(-3.5, -2.2) if model == 1 else None, rng.uniform(50.0, 2000.0) * KEV, cen) for _ in range(256)])
    mu = shapes * np.diff(edges)
    mu *= total / mu.sum(axis=1, keepdims=True)
    count = rng.poisson(mu[np.arange(n_spec) % 256]).astype(np.int64)
    return edges, count, count * 1e50


def child(args):
    from mcrat_amd import engine, synth
    engine.load_library()
    n_spec, n_e, model = (int(x) for x in args.child.split(","))
    name = "band" if model else "comp"
    edges, count, w = spectra(model, n_spec, n_e)
    e = engine.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    if args.step == "calls":
        ts, res = [], None
        for k in range(args.reps + 1):
            t0 = time.perf_counter()
            res = e.fit_spectra(count, w, edges, model=model)
            if k:
                ts.append((time.perf_counter() - t0) * 1e3)
        fitted = int(((res["status"] & (engine.FIT_TOO_FEW_BINS | engine.FIT_NO_FINITE_CANDIDATE)) == 0).sum())
        at_bound = int(((res["status"] & (engine.FIT_AT_BOUND_ALPHA | engine.FIT_AT_BOUND_LAMBDA | engine.FIT_AT_BOUND_BETA)) != 0).sum())
        print("RESULT spectra=%d bins=%d model=%s call_ms=%.1f(%.1f,%.1f) reps=%d fitted=%d at_bound=%d median_red_chi2=%.3f" % (
            n_spec, n_e, name, np.median(ts), min(ts), max(ts), args.reps, fitted, at_bound, float(np.nanmedian(res["chi2"] / res["dof"]))), flush=True)
    else:
        m = min(args.host_spectra, n_spec)
        res = e.fit_spectra(count[:m], w[:m], edges, model=model)
        t0 = time.perf_counter()
        want = F.fit(count[:m], w[:m], edges, F.log_e_of(edges), model, F.default_bounds(edges))
        host = time.perf_counter() - t0
        same = all(np.asarray(want[k]).tobytes() == np.ascontiguousarray(res[k]).tobytes() for k in ("alpha", "beta", "e_peak", "amplitude", "chi2"))
        print("CHECKER spectra=%d bins=%d model=%s checker_s_on_%d=%.2f checker_s_scaled_to_all=%.0f same_bits=%s" % (n_spec, n_e, name, m, host, host * n_spec / m, same),
              flush=True)
    e.close()


def start(args, case, step, limit, profiler=None):
    """a fresh process of this script for one step of one case, its output passed through; nothing more is started on the GPU after one that failed"""
    timeout = shutil.which("timeout")
    cmd = ([timeout, "-k", "10", str(limit)] if timeout else []) + (profiler or []) + [sys.executable, os.path.abspath(__file__), "--child", case, "--step", step,
           "--reps", str(args.reps), "--host-spectra", str(args.host_spectra)]
    r = subprocess.run(cmd, stderr=subprocess.PIPE if profiler else None, text=True)       # (the profiler's own chatter is shown only when the step failed)
    if r.returncode:
        sys.stderr.write((r.stderr or "")[-3000:])
        sys.exit("exit %d (124, 137: the limit of %d s): %s" % (r.returncode, limit, " ".join(cmd)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="(internal) n_spec,n_e,model: one step of this case in this process")
    ap.add_argument("--step", default="calls", choices=("calls", "checker"), help="(internal)")
    ap.add_argument("--trace", action="store_true", help="run the calls under rocprofv3 for the kernel time")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-spectra", type=int, default=32, help="spectra the NumPy checker is timed on (0: not timed)")
    ap.add_argument("--sizes", default="10000,600000", help="ascending")
    ap.add_argument("--bins", default="64,128")
    ap.add_argument("--limit", type=int, default=300, help="seconds one process may take")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.trace and shutil.which("rocprofv3") is None:
        sys.exit("rocprofv3 is needed for the kernel times")
    sizes = [int(s) for s in args.sizes.split(",")]
    seen = {}                                                              # (bins, model) -> (spectra, seconds a call took) at the size before
    for size in sizes:
        for n_e in (int(s) for s in args.bins.split(",")):
            for model in (1, 0):
                case, name = "%d,%d,%d" % (size, n_e, model), "band" if model else "comp"
                if (n_e, model) in seen:
                    before, secs = seen[(n_e, model)]
                    predicted = secs * size / before * (args.reps + 1)
                    if predicted > 0.5 * args.limit:
                        print("SKIPPED spectra=%d bins=%d model=%s predicted_s=%.0f limit_s=%d (from %d spectra)" % (size, n_e, name, predicted, args.limit, before), flush=True)
                        continue
                d = tempfile.mkdtemp(prefix="fit_trace_") if args.trace else None
                t0 = time.perf_counter()
                start(args, case, "calls", args.limit, profiler=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] if d else None)
                secs = (time.perf_counter() - t0) / (args.reps + 1)        # an upper bound for one call: the process's start is in it
                if d:
                    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                        for row in csv.DictReader(open(f)):
                            if re.search(r"fit_kernel", row["Name"]):
                                secs = float(row["AverageNs"]) / 1e9
                                print("KERNEL spectra=%d bins=%d model=%s calls=%s avg_ms=%.2f min_ms=%.2f max_ms=%.2f fit_kernel" % (
                                    size, n_e, name, row["Calls"], float(row["AverageNs"]) / 1e6, float(row["MinNs"]) / 1e6, float(row["MaxNs"]) / 1e6), flush=True)
                    shutil.rmtree(d, ignore_errors=True)
                seen[(n_e, model)] = (size, secs)
                if size == sizes[0] and args.host_spectra > 0:
                    start(args, case, "checker", args.limit)


if __name__ == "__main__":
    main()
