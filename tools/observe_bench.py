"""Mock observations on the device against the host route, on bench.py's headline pool (cfg2, 1e6 photons as 1025 ragged lists, one frame propagated):
    python tools/observe_bench.py [--reps 20] [--host-reps 3] [--only large|small-lds|small-global] [--no-host] [--nzc 64] [--photons 1000000]
    python tools/observe_bench.py --kernels            kernel times, bytes over time, share of the 8 TB/s peak
    python tools/observe_bench.py --counters           the L2's atomic counters for the global path
Times mcrat_hip_pool_observe (a host clock around the call, which ends in a stream synchronise) for
    large    16 observers x 256 time bins x 64 energy bins: beyond LDS, the global path
    small    1 observer x 1 x 64: the LDS path, and the global path forced (MCRAT_HIP_OBSERVE_PATH)
each with every plane read back and with none (the counters only: memset + copy of the inputs + the kernel), and beside it the only route to the
same cube without the entry point: mcrat_hip_get_photons_soa of the needed columns, list by list, and the binning in NumPy on the host.  The device
cube must equal the host's: counts exactly, sums to 1e-12 of a bin's sum of |terms|.  Prints the bytes the pass reads, from the shapes (10 B per slot
for flags, type and weight, 72 B more per observable photon with Stokes on, 40 B without).
--kernels and --counters take no times themselves: each starts, per variant, a fresh process of this script (--only, --no-host) under rocprofv3 --
a kernel trace with statistics, or the counters in a run of their own -- and reads observe_kernel's rows from what the profiler wrote: the kernel's
time, the pass's bytes over it as a share of the HBM peak; the atomic requests that left L2, at 64 B each, over the kernel time of the trace."""
import argparse
import csv
import ctypes as C
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcrat_amd import engine, synth  # noqa: E402

SEED = 0x4D435261
C_LIGHT = 2.99792458e10
HBM_PEAK = 8.0e12
VARIANTS = ("large", "small-lds", "small-global")
ATOMIC_COUNTERS = ("TCC_EA0_ATOMIC_sum", "TCC_ATOMIC_sum", "TCC_EA0_ATOMIC_LEVEL_sum", "TCC_EA0_RDREQ_sum")      # the TCC's four slots: one pass
PLANES = (("w", None), ("we", "e"), ("i", "s0"), ("q", "s1"), ("u", "s2"), ("v", "s3"))
_dp = C.POINTER(C.c_double)


def layout(n, rank_photons=976):
    """bench.py's list lengths (its list_layout at the default --rank-photons: a function inside its main(), so restated here, not imported)"""
    k = max(1, int(round(n / float(rank_photons))))
    ln = np.full(k, n // k, dtype=np.int64)
    ln[: n - int(ln.sum())] += 1
    if k > 1 and ln.min() > 80:
        d = np.random.default_rng(SEED).integers(-40, 41, k // 2)
        ln[: 2 * (k // 2): 2] += d
        ln[1: 2 * (k // 2): 2] -= d
    return k, ln, np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)


def needed_columns(view, stokes):
    """mcrat_hip_get_photons_soa of the columns an observation reads, nothing else"""
    n = view.n
    names = ["p0", "p3", "r0", "r1", "r2", "weight"] + (["s0", "s1", "s2", "s3"] if stokes else [])
    out, s = {k: np.empty(n) for k in names}, engine.PhotonSoA()
    s.n = n
    for k in names:
        setattr(s, k, out[k].ctypes.data_as(_dp))
    out["type"] = np.empty(n, dtype="S1")
    s.type = out["type"].ctypes.data_as(C.c_char_p)
    view._check(view.lib.mcrat_hip_get_photons_soa(view.ctx, C.byref(s)), "get_photons_soa")
    return out


def find_bin(edges, x):
    k = np.searchsorted(edges, x, side="right") - 1
    return np.where((k >= 0) & (k < len(edges) - 1), k, -1)


def host_cube(ph, clocks, obs, t_edges, e_edges, stokes):
    """the definitions of include/mcrat_hip.h in NumPy; the sums by np.bincount"""
    co, so, cl, ch = obs
    n_obs, n_t, n_e = len(co), len(t_edges) - 1, len(e_edges) - 1
    p0, p3, r0, r1, r2, w = (ph[k] for k in ("p0", "p3", "r0", "r1", "r2", "weight"))
    observable = (w != 0) & (ph["type"] != b"p") & (ph["type"] != b"N")
    e = p0 * C_LIGHT
    ie = find_bin(e_edges, e)
    rho = np.sqrt(r0 * r0 + r1 * r1)
    terms = {"w": w, "we": w * e}
    for k, col in PLANES[2:]:
        terms[k] = w * ph[col] if stokes else None
    res = {"count": np.zeros((n_obs, n_t * n_e), dtype=np.int64), "n_accepted": np.zeros(n_obs, dtype=np.int64), "n_outside": np.zeros(n_obs, dtype=np.int64)}
    for k, _ in PLANES:
        res[k], res["abs_" + k] = np.zeros((n_obs, n_t * n_e)), np.zeros((n_obs, n_t * n_e))
    for o in range(n_obs):
        acc = observable & (p3 <= p0 * cl[o]) & (p3 > p0 * ch[o])
        idx = np.nonzero(acc)[0]
        t = clocks[idx] - ((r2[idx] * co[o] + rho[idx] * so[o]) / C_LIGHT)
        it, je = find_bin(t_edges, t), ie[idx]
        inside = (it >= 0) & (je >= 0)
        flat, idx = (it * n_e + je)[inside], idx[inside]
        res["n_accepted"][o], res["n_outside"][o] = len(acc.nonzero()[0]), int((~inside).sum())
        res["count"][o] = np.bincount(flat, minlength=n_t * n_e)
        for k, _ in PLANES:
            if terms[k] is not None:
                res[k][o] = np.bincount(flat, weights=terms[k][idx], minlength=n_t * n_e)
                res["abs_" + k][o] = np.bincount(flat, weights=np.abs(terms[k][idx]), minlength=n_t * n_e)
    for k in ("count",) + tuple(k for k, _ in PLANES) + tuple("abs_" + k for k, _ in PLANES):
        res[k] = res[k].reshape(n_obs, n_t, n_e)
    return res


def observe_raw(pool, obs, t_edges, e_edges, clocks, planes):
    """mcrat_hip_pool_observe with the planes read back or not (the per-observer counters always)"""
    if planes:
        return pool.pool_observe(*obs, t_edges, e_edges, clocks)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in obs + (t_edges, e_edges, clocks)]
    o = engine.Observer(len(arrs[0]), *[a.ctypes.data_as(_dp) for a in arrs[:4]], len(t_edges) - 1, arrs[4].ctypes.data_as(_dp), len(e_edges) - 1,
                        arrs[5].ctypes.data_as(_dp))
    acc, outside = np.zeros(len(arrs[0]), dtype=np.int64), np.zeros(len(arrs[0]), dtype=np.int64)
    ll = C.POINTER(C.c_longlong)
    out = engine.Observation(None, None, None, None, None, None, None, acc.ctypes.data_as(ll), outside.ctypes.data_as(ll))
    pool._check(pool.lib.mcrat_hip_pool_observe(pool.ctx, C.byref(o), arrs[6].ctypes.data_as(_dp), C.byref(out)), "pool_observe")
    return {"n_accepted": acc, "n_outside": outside}


def timed(fn, reps, warm=3):
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


def profiled(only, args, profiler):
    """a fresh process of this script for one variant under rocprofv3; what it printed, and the folder the profiler wrote into"""
    d = tempfile.mkdtemp(prefix="observe_%s_" % only)
    cmd = ["timeout", "-k", "10", "600", "rocprofv3"] + profiler + ["--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--only", only, "--no-host", "--reps", str(args.reps), "--photons", str(args.photons), "--nzc", str(args.nzc), "--stokes", str(args.stokes),
           "--frames", str(args.frames)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s\n%s\nexit %d: %s" % (r.stdout[-2000:], r.stderr[-2000:], r.returncode, " ".join(cmd)))
    return r.stdout, d


def pass_bytes_of(text):
    return int(re.search(r"pass_bytes=(\d+)", text).group(1))


def kernel_stats(d):
    """observe_kernel's row of the profiler's kernel statistics: name, calls, average, min, max [us]"""
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "observe_kernel" in row["Name"]:
                return (row["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void mcrat::", ""), int(row["Calls"]),
                        float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3)
    sys.exit("no observe_kernel in the kernel statistics under " + d)


def kernels(args):
    times = {}
    print("%-13s %-28s %5s %10s %10s %10s %14s %16s" % ("variant", "kernel", "calls", "avg us", "min us", "max us", "bytes / time", "share of 8 TB/s"))
    for only in VARIANTS:
        text, d = profiled(only, args, ["--kernel-trace", "--stats"])
        name, calls, avg, lo, hi = kernel_stats(d)
        rate = pass_bytes_of(text) / (avg * 1e-6)
        times[only] = avg
        print("%-13s %-28s %5d %10.1f %10.1f %10.1f %9.1f GB/s %14.2f %%" % (only, name, calls, avg, lo, hi, rate / 1e9, 100.0 * rate / HBM_PEAK), flush=True)
    return times


def counters(args):
    """The L2's atomic counters per dispatch of observe_kernel on the global path, in a run of their own; the kernel time from a kernel trace of its
    own (a counter run stretches the kernel).  Requests x 64 B over that time is what to hold against a chip-wide rate of memory-side atomics."""
    for only in ("large", "small-global"):
        text, d = profiled(only, args, ["--kernel-trace", "--stats"])
        _, _, avg, _, _ = kernel_stats(d)
        text, d = profiled(only, args, ["--pmc"] + list(ATOMIC_COUNTERS))
        acc = {}
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "observe_kernel" in row["Kernel_Name"]:
                    acc.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
        if not acc:
            sys.exit("no observe_kernel in the counters under " + d)
        print("%-13s kernel %.1f us (kernel trace); per dispatch, median of %d:" % (only, avg, len(next(iter(acc.values())))))
        med = {k: statistics.median(v) for k, v in acc.items()}
        for k in sorted(med):
            print("    %-26s %14.0f   (min %.0f, max %.0f)" % (k, med[k], min(acc[k]), max(acc[k])))
        m = re.search(r"binned_pairs=(\d+)", text)
        if m and "TCC_EA0_ATOMIC_sum" in med:
            ea = med["TCC_EA0_ATOMIC_sum"]
            print("    %d binned (photon, observer) pairs x 7 planes = %d adds before a wavefront combines; %.3f requests out of L2 per such add" %
                  (int(m.group(1)), 7 * int(m.group(1)), ea / (7.0 * int(m.group(1)))))
            print("    requests x 64 B / kernel time = %.1f GB/s;  x 8 B (the bytes added) = %.1f GB/s" % (ea * 64 / (avg * 1e-6) / 1e9, ea * 8 / (avg * 1e-6) / 1e9))
            if med.get("TCC_EA0_ATOMIC_LEVEL_sum"):
                print("    atomics in flight / atomics = %.0f L2 cycles each on the way out and back" % (med["TCC_EA0_ATOMIC_LEVEL_sum"] / ea))
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="kernel times of the three variants from kernel traces of fresh processes; nothing else")
    ap.add_argument("--counters", action="store_true", help="the L2's atomic counters on the global path, from counter runs of fresh processes; nothing else")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--only", choices=("large", "small-lds", "small-global"), default=None, help="one variant, with the planes read back (for a kernel trace)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--photons", type=int, default=1_000_000)
    ap.add_argument("--nzc", type=int, default=64)
    ap.add_argument("--stokes", type=int, default=1)
    ap.add_argument("--frames", type=int, default=1, help="hydro frames propagated before the observation (0: the photons as injected)")
    args = ap.parse_args()
    if args.kernels or args.counters:          # this process never opens the GPU: its children do, one at a time
        if args.kernels:
            kernels(args)
        if args.counters:
            counters(args)
        return

    frame, ph, cfg = synth.config2(n_photons=args.photons, seed=SEED, nzc=args.nzc, stokes=args.stokes)
    n = int(ph["p0"].size)
    R, lens, offs = layout(n)
    pool = engine.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    pool.set_hydro(frame)
    pool.pool_create(R, int(lens.max()))
    views = [pool.pool_rank(r, r) for r in range(R)]
    recs = synth.photons_to_aos(ph, engine.PHOTON_DTYPE)
    pool.pool_set_photons(list(range(R)), [recs[int(offs[r]):int(offs[r + 1])] for r in range(R)])
    remaining = 1.0 / frame["fps"]
    for k in range(args.frames):
        pool.begin_frame(1000 + k, k * remaining, remaining)
        st = pool.run(0)
        print("frame %d: %d scatterings, %d passes" % (k, st.frame_scatt_cnt, st.iterations), flush=True)
    # every list its own clock, as the ranks of a run have: spread over one frame
    clocks = args.frames * remaining + remaining * np.arange(R) / R
    slots = int(pool.n)

    # observers and edges from the photons themselves: percentiles of the directions, the detection times and the energies
    def columns():
        per = [needed_columns(v, args.stokes) for v in views]
        return {k: np.concatenate([p[k] for p in per]) for k in per[0]}
    cat = columns()
    per_photon_clock = np.repeat(clocks, lens)
    theta = np.arccos(np.clip(cat["p3"] / cat["p0"], -1.0, 1.0))
    centres = np.percentile(theta, np.linspace(5, 95, 16))
    big = engine.observer_angles(np.degrees(centres), np.degrees(np.full(16, 2.0 * (centres[1] - centres[0]))))        # neighbours overlap
    one = engine.observer_angles([np.degrees(centres[8])], [np.degrees(np.percentile(theta, 90))])
    t_mid = per_photon_clock - (cat["r2"] * big[0][8] + np.sqrt(cat["r0"] ** 2 + cat["r1"] ** 2) * big[1][8]) / C_LIGHT
    t256 = np.linspace(np.percentile(t_mid, 1), np.percentile(t_mid, 99), 257)
    e_all = cat["p0"] * C_LIGHT
    e64 = 10.0 ** np.linspace(np.log10(np.percentile(e_all, 1)), np.log10(np.percentile(e_all, 99)), 65)
    t1 = np.array([t256[0], t256[-1]])
    observable = int(((cat["weight"] != 0) & (cat["type"] != b"p") & (cat["type"] != b"N")).sum())
    pass_bytes = slots * 10 + observable * (72 if args.stokes else 40)
    print("pool: %d lists, %d slots, %d observable photons; the pass reads %.1f MB (%.1f us at the 8 TB/s peak, derived) pass_bytes=%d" %
          (R, slots, observable, pass_bytes / 1e6, pass_bytes / HBM_PEAK * 1e6, pass_bytes), flush=True)

    variants = {"large": (big, t256, e64, None), "small-lds": (one, t1, e64, "lds"), "small-global": (one, t1, e64, "global")}

    def forced(path):
        if path is None:
            os.environ.pop("MCRAT_HIP_OBSERVE_PATH", None)
        else:
            os.environ["MCRAT_HIP_OBSERVE_PATH"] = path

    if args.only:
        obs, te, ee, path = variants[args.only]
        forced(path)
        ts = timed(lambda: observe_raw(pool, obs, te, ee, clocks, True), args.reps)
        print("%-13s path %d, all planes read back: %s" % (args.only, pool.observe_path(), fmt(ts)))
        res = pool.pool_observe(*obs, te, ee, clocks)
        print("binned_pairs=%d bins_in_use=%d" % (int(res["count"].sum()), int((res["count"] > 0).sum())))
        pool.close()
        return

    # device against host, once per cube
    results = {}
    for name in VARIANTS:
        obs, te, ee, path = variants[name]
        forced(path)
        results[name] = pool.pool_observe(*obs, te, ee, clocks)
        print("%-13s path %d: %d accepted, %d outside, %d bins of %d in use" % (name, pool.observe_path(), results[name]["n_accepted"].sum(),
              results[name]["n_outside"].sum(), int((results[name]["count"] > 0).sum()), results[name]["count"].size), flush=True)
    if not args.no_host:
        for name in VARIANTS:
            obs, te, ee, _ = variants[name]
            want = host_cube(cat, per_photon_clock, obs, te, ee, args.stokes)
            for k in ("count", "n_accepted", "n_outside"):
                assert np.array_equal(results[name][k], want[k]), (name, k)
            for k, _ in PLANES:
                assert (np.abs(results[name][k] - want[k]) <= 1e-12 * want["abs_" + k]).all(), (name, k)
        print("device cubes equal the host's: counts exactly, sums to 1e-12 of the bin's sum of |terms|", flush=True)

    # timings: the variants in turn, round after round, so that whatever else the machine does hits all of them alike
    calls = {}
    for name in VARIANTS:
        obs, te, ee, path = variants[name]
        for planes in (True, False):
            calls[(name, planes)] = (lambda obs=obs, te=te, ee=ee, path=path, planes=planes: (forced(path), observe_raw(pool, obs, te, ee, clocks, planes)))
    for fn in calls.values():
        for _ in range(3):
            fn()
    ts = {key: [] for key in calls}
    for _ in range(args.reps):
        for key, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ts[key].append((time.perf_counter() - t0) * 1e3)
    for (name, planes), v in ts.items():
        print("pool_observe %-13s %-22s %s" % (name, "all planes read back:" if planes else "counters only:", fmt(v)))
    forced(None)
    if not args.no_host:
        t_get = timed(columns, args.host_reps, warm=1)
        print("host route, get_photons_soa of the needed columns, %d lists: %s" % (R, fmt(t_get)))
        for name in ("large", "small-lds"):
            obs, te, ee, _ = variants[name]
            t_bin = timed(lambda: host_cube(cat, per_photon_clock, obs, te, ee, args.stokes), args.host_reps, warm=1)
            print("host route, NumPy binning, %-10s %s" % (name.split("-")[0] + ":", fmt(t_bin)))
    pool.close()


if __name__ == "__main__":
    main()
