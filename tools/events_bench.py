"""Detected-photon event lists on the device: both orders against each other, against the sky observation of the same observers, and against the
read-back route, on synthetic lists:
    python tools/events_bench.py [--reps 10] [--host-reps 2] [--sizes 1000000,10000000] [--trace]
It never opens the GPU itself: it starts a fresh process per list size, one at a time, checks every exit status and prints what they measured.
The lists: a jet about the r2 axis that is not axisymmetric (r ~ 1e12 .. 1e13 cm within 0.5 rad of the axis, every photon within ~0.15 rad of its
radial direction, p0 over six decades), Stokes on, generated from a seed.  The cases: one observer at (theta, phi) = (0.2, 0) and 16 observers on
the ring theta = 0.2, each with a cone of 1 degree, of 10 degrees, and with everything accepted (cos_acc = -1).  Everything accepted is measured
with one observer at every size and with 16 observers at 1e6 photons only: 16 x 1e7 rows are 16 GB on the device and 14 GB to read back.
Per case, in turn, round after round:
    by-photon   mcrat_hip_observe_events, MCRAT_HIP_EVENTS_BY_PHOTON, capacity = n_total (known from a counting call outside the timed window)
    by-time     ... MCRAT_HIP_EVENTS_BY_TIME, with the sort passes that ran and those that were skipped
    count       the counting call alone (capacity 0): count kernel and scan
    sky         mcrat_hip_observe_sky of the same observers on 32 t x 32 e bins: the yardstick of a binned product
    read-back   mcrat_hip_get_photons_soa of the needed columns and NumPy: acceptance per observer, np.lexsort on (slot, key, observer), the columns
                gathered; its rows must equal the device's (t, slot, w bit for bit)
Call time: a host clock around the call, which ends in a stream synchronise (memset, copy of the inputs, the kernels, every column read back);
median, min and max of --reps calls after three warm-up calls each.  --trace adds one run per size under rocprofv3 --kernel-trace --stats, in a
process of its own, and prints the rows of this product's kernels and of sky_kernel.  Needs nothing outside the repository."""
import argparse
import csv
import ctypes as C
import glob
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C_LIGHT = 2.99792458e10
SEED = 20261021
TIME_NOW = 400.0
BY_PHOTON, BY_TIME = 0, 1
_dp = C.POINTER(C.c_double)
COLS = ["p0", "p1", "p2", "p3", "r0", "r1", "r2", "weight", "s0", "s1", "s2", "s3", "num_scatt"]


def jet(n, seed=SEED, opening=0.5):
    g = np.random.default_rng(seed)
    r = 10.0 ** g.uniform(12.0, 13.0, n)
    th = opening * np.sqrt(g.uniform(0.0, 1.0, n))
    phi = np.where(g.uniform(0, 1, n) < 2.0 / 3.0, g.normal(0.0, 1.0, n), g.uniform(0.0, 2 * np.pi, n))
    rhat = np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)])
    d = rhat + 0.1 * g.standard_normal((3, n))
    d /= np.sqrt((d * d).sum(axis=0))
    p0 = 10.0 ** g.uniform(-20.0, -14.0, n)
    pv = p0 * d
    ph = {"r0": r * rhat[0], "r1": r * rhat[1], "r2": r * rhat[2], "p0": np.sqrt((pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2]), "p1": pv[0], "p2": pv[1],
          "p3": pv[2], "s0": np.ones(n), "s1": g.uniform(-1.0, 1.0, n), "s2": g.uniform(-1.0, 1.0, n), "s3": g.uniform(-1.0, 1.0, n),
          "weight": 10.0 ** g.uniform(48.0, 51.0, n), "num_scatt": np.floor(g.uniform(0.0, 30.0, n)), "time_to_scatter": np.zeros(n),
          "total_optical_depth": np.ones(n), "type": np.full(n, b"i", dtype="S1"), "nearest_block_index": np.zeros(n, dtype=np.int32),
          "recalc_properties": np.ones(n, dtype=np.int32)}
    for k in ("comv_p0", "comv_p1", "comv_p2", "comv_p3"):
        ph[k] = ph[k[5:]].copy()
    return ph


def key(t):
    bits = np.ascontiguousarray(t, dtype=np.float64).view(np.uint64)
    sign = np.uint64(1 << 63)
    return np.where((bits & sign) != 0, ~bits, bits | sign)


def host_list(cat, n, cos_acc):
    """the BY_TIME list from read-back columns: acceptance per observer, one lexsort, the columns gathered"""
    p0, p1, p2, p3, r0, r1, r2, w = (cat[k] for k in ("p0", "p1", "p2", "p3", "r0", "r1", "r2", "weight"))
    observable = (w != 0) & (cat["type"] != b"p") & (cat["type"] != b"N")
    obs, idx, ts = [], [], []
    for o in range(n.shape[1]):
        i = np.nonzero(observable & (((p1 * n[0, o] + p2 * n[1, o]) + p3 * n[2, o]) >= p0 * cos_acc[o]))[0]
        idx.append(i)
        obs.append(np.full(len(i), o))
        ts.append(TIME_NOW - (((r0[i] * n[0, o] + r1[i] * n[1, o]) + r2[i] * n[2, o]) / C_LIGHT))
    obs, idx, ts = np.concatenate(obs), np.concatenate(idx), np.concatenate(ts)
    by = np.lexsort((idx, key(ts), obs))
    idx = idx[by]
    res = {"t": ts[by], "slot": idx.astype(np.int32), "e": p0[idx] * C_LIGHT, "w": w[idx], "type": cat["type"][idx]}
    for k in ("s0", "s1", "s2", "s3", "num_scatt"):
        res[k] = cat[k][idx]
    return res


def child(args):
    """one process with the GPU open: one list, the cases in turn"""
    from mcrat_amd import engine, synth
    n_ph = int(args.child)
    e = engine.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    e.set_photons(jet(n_ph))
    print("list: %d photons" % n_ph, flush=True)
    te, ee = np.linspace(0.0, 400.0, 33), 10.0 ** np.linspace(-10.0, -3.0, 33)
    only = [c for c in args.cases.split(",") if c]

    def columns():
        out, s = {k: np.empty(e.n) for k in COLS}, engine.PhotonSoA()
        s.n = e.n
        for k in COLS:
            setattr(s, k, out[k].ctypes.data_as(_dp))
        out["type"] = np.empty(e.n, dtype="S1")
        s.type = out["type"].ctypes.data_as(C.c_char_p)
        e._check(e.lib.mcrat_hip_get_photons_soa(e.ctx, C.byref(s)), "get_photons_soa")
        return out

    def timed(f, reps, warm=3):
        for _ in range(warm):
            f()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    fmt = lambda ts: "%.3f (%.3f, %.3f)" % (statistics.median(ts), min(ts), max(ts))
    for n_obs in (1, 16):
        for cone in ("1deg", "10deg", "all"):
            name = "%dobs-%s" % (n_obs, cone)
            if only and name not in only:
                continue
            if cone == "all" and n_obs == 16 and n_ph > 1_000_000:
                print("RESULT case=%s photons=%d skipped=rows_beyond_16GB" % (name, n_ph), flush=True)
                continue
            half = {"1deg": np.radians(1.0), "10deg": np.radians(10.0), "all": np.pi}[cone]
            n, cos_acc, ex, ey = engine.sky_observers(np.full(n_obs, 0.2), 2 * np.pi * np.arange(n_obs) / n_obs, np.full(n_obs, half))
            if cone == "all":
                cos_acc = -np.ones(n_obs)
            first = e.observe_events(n, cos_acc, TIME_NOW, BY_TIME)
            total = first["n_total"]
            calls = {"by-photon": lambda: e.observe_events(n, cos_acc, TIME_NOW, BY_PHOTON, capacity=total),
                     "by-time": lambda: e.observe_events(n, cos_acc, TIME_NOW, BY_TIME, capacity=total),
                     "count": lambda: count_only(e, engine, n, cos_acc),
                     "sky": lambda: e.observe_sky(n, cos_acc, te, ee, TIME_NOW)}
            ts = {k: [] for k in calls}
            for k, f in calls.items():
                for _ in range(3):
                    f()
            for _ in range(args.reps):
                for k, f in calls.items():
                    t0 = time.perf_counter()
                    f()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
            sky = e.observe_sky(n, cos_acc, te, ee, TIME_NOW)
            assert np.array_equal(sky["n_accepted"], first["n_accepted"]), name
            host = ""
            if args.host_reps > 0:
                def route():
                    return host_list(columns(), n, cos_acc)
                want = route()
                for k in ("t", "slot", "w", "e", "num_scatt"):
                    assert want[k].tobytes() == first[k].tobytes(), (name, k)
                host = fmt(timed(route, args.host_reps, warm=0))
            print("RESULT case=%s photons=%d rows=%d passes_run=%d passes_skipped=%d by_photon_ms=%s by_time_ms=%s count_ms=%s sky_ms=%s readback_ms=%s" %
                  (name, n_ph, total, first["sort_passes_run"], first["sort_passes_skipped"], fmt(ts["by-photon"]).replace(" ", ""), fmt(ts["by-time"]).replace(" ", ""),
                   fmt(ts["count"]).replace(" ", ""), fmt(ts["sky"]).replace(" ", ""), host.replace(" ", "") or "not_measured"), flush=True)
    e.close()


def count_only(e, engine, n, cos_acc):
    """the counting call through the ABI: capacity 0, no row pointer"""
    sky, _alive, _, _ = e._sky_observer("observe_events", n, cos_acc, [0.0, 1.0], [0.0, 1.0], None, None, None, None)
    obs = engine.EventsObserver(sky.n_obs, sky.n0, sky.n1, sky.n2, sky.cos_acc, None, None, None, None, None, None, -np.inf, np.inf, -np.inf, np.inf, BY_TIME, 0, 0)
    out = engine.Events()
    e._check(e.lib.mcrat_hip_observe_events(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)), "observe_events")
    return int(out.n_total)


def start(args, size, profiler=None, cases=""):
    """a fresh process of this script for one list; nothing more is started on the GPU after one that failed"""
    timeout = shutil.which("timeout")
    cmd = ([timeout, "-k", "10", str(args.limit)] if timeout else []) + (profiler or []) + [sys.executable, os.path.abspath(__file__), "--child", str(size),
           "--reps", str(args.reps if not profiler else 3), "--host-reps", str(args.host_reps if not profiler else 0), "--cases", cases]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s\n%s\nexit %d: %s" % (r.stdout[-3000:], r.stderr[-3000:], r.returncode, " ".join(cmd)))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="(internal) measure a list of this many photons in this process")
    ap.add_argument("--cases", default="", help="only these cases, comma-separated (1obs-1deg, 16obs-all, ...)")
    ap.add_argument("--trace", action="store_true", help="also one run per size under rocprofv3 for the kernel times")
    ap.add_argument("--trace-case", default="16obs-10deg", help="the case the traced run measures")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--limit", type=int, default=540, help="seconds a child may take")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for size in (int(s) for s in args.sizes.split(",")):
        print("---- call times, %d photons" % size, flush=True)
        text = start(args, size, cases=args.cases)
        sys.stdout.write(text)
        rows += [dict(kv.split("=") for kv in line.split()[1:]) for line in text.splitlines() if line.startswith("RESULT")]
        if args.trace:
            if shutil.which("rocprofv3") is None:
                sys.exit("rocprofv3 is needed for the kernel times")
            d = tempfile.mkdtemp(prefix="events_trace_")
            print("---- kernel trace, %d photons, %s" % (size, args.trace_case), flush=True)
            start(args, size, profiler=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"], cases=args.trace_case)
            for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    hit = re.search(r"(events_\w+_kernel|sky_kernel)(<[^(]*>)?", row["Name"])
                    if hit:
                        print("KERNEL photons=%d calls=%s avg_us=%.1f min_us=%.1f max_us=%.1f %s" % (size, row["Calls"], float(row["AverageNs"]) / 1e3,
                              float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3, hit.group(0).replace(" ", "")), flush=True)
            shutil.rmtree(d, ignore_errors=True)
    print("---- summary: whole calls [ms], median (min, max)")
    print("%-9s %-11s %-10s %-7s %-26s %-26s %-24s %-24s %s" % ("photons", "case", "rows", "passes", "by-photon", "by-time", "count only", "observe_sky", "read-back + NumPy"))
    for r in rows:
        if "skipped" in r:
            print("%-9s %-11s not measured: %s" % (r["photons"], r["case"], r["skipped"]))
            continue
        print("%-9s %-11s %-10s %-7s %-26s %-26s %-24s %-24s %s" % (r["photons"], r["case"], r["rows"], "%s+%s" % (r["passes_run"], r["passes_skipped"]),
              r["by_photon_ms"], r["by_time_ms"], r["count_ms"], r["sky_ms"], r["readback_ms"]))


if __name__ == "__main__":
    main()
