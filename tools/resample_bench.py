"""Resampled sky observations on the device: the accumulation paths against each other, against the sky observation they extend, and against the
read-back route, on bench.py's headline pool (cfg2: 1e6 photons as 1025 ragged lists, Stokes on, one frame propagated):
    python tools/resample_bench.py [--reps 20] [--host-reps 2] [--photons 1000000] [--nzc 64] [--no-trace] [--no-sweep]
It never opens the GPU itself: it starts fresh processes one at a time, checks every exit status and prints what they measured.
The variants (one observer on the axis, its cone the 90th percentile of the photons' polar angles; edges from percentiles, as tools/sky_bench.py):
    sky            mcrat_hip_pool_observe_sky on 1 x 32 t x 32 e, its LDS path: the yardstick
    none-stored    NONE / AS_STORED on the same shape: the same cube through the new kernel
    none-plane     NONE / SKY_PLANE on the same shape: what the rotation costs
    jk32-sliced    JACKKNIFE, 32 groups, SKY_PLANE on the same shape: 32 slices of one group each in LDS
    jk32-global    ... the same cube with atomics in HBM
    boot-sliced    BOOTSTRAP, the sample and 200 replicas, SKY_PLANE on 1 x 8 t x 16 e: 19 slices of 11 entries
    boot-global    ... the same cube with atomics in HBM
    image-sliced   JACKKNIFE, 16 groups, SKY_PLANE on 1 x 1 x 1 x 36 x 36 pixels: 16 slices of one group each
    image-global   ... the same cube with atomics in HBM
    jkG-sliced, jkG-global for G = 8, 128, 512 (the sweep): where the answer between the two changes with the number of slices
Call time: a host clock around the call, which ends in a stream synchronise (memset, copy of the inputs, kernel, the seven planes read back); the
variants in turn, round after round; median, min and max of --reps calls after three warm-up calls each.  Kernel time: the kernel's row of
rocprofv3 --kernel-trace --stats, in runs of their own (a child traces only variants whose kernels differ in name), average, min and max over the
same calls.  Beside them, once per variant, the only route to the same cubes without the entry point: mcrat_hip_get_photons_soa of the needed
columns list by list and the definitions in NumPy -- Philox, the multiplicities, the rotation, np.bincount per replica; the device's cubes must
equal that route's (counts exactly, sums to 1e-12 of a bin's sum of |terms|).  Needs nothing outside the repository."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sky_bench                                     # noqa: E402  (bench.py's list layout, find_bin, the timing helpers)

C_LIGHT = 2.99792458e10
NONE, JACKKNIFE, BOOTSTRAP = 0, 1, 2
AS_STORED, SKY_PLANE = 0, 1
SEED = 20261021
THRESHOLDS = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463, 4294966817, 4294967252,
              4294967292)
SUMS = ("w", "we", "i", "q", "u", "v")
SWEEP = (8, 128, 512)
# variant: (shape, mode, n_rep, frame, forced path or None)
VARIANTS = {"sky": ("d", None, 1, AS_STORED, None), "none-stored": ("d", NONE, 1, AS_STORED, None), "none-plane": ("d", NONE, 1, SKY_PLANE, None),
            "jk32-sliced": ("d", JACKKNIFE, 32, SKY_PLANE, "sliced"), "jk32-global": ("d", JACKKNIFE, 32, SKY_PLANE, "global"),
            "boot-sliced": ("f", BOOTSTRAP, 201, SKY_PLANE, "sliced"), "boot-global": ("f", BOOTSTRAP, 201, SKY_PLANE, "global"),
            "image-sliced": ("e", JACKKNIFE, 16, SKY_PLANE, "sliced"), "image-global": ("e", JACKKNIFE, 16, SKY_PLANE, "global")}
for _G in SWEEP:
    VARIANTS["jk%d-sliced" % _G] = ("d", JACKKNIFE, _G, SKY_PLANE, "sliced")
    VARIANTS["jk%d-global" % _G] = ("d", JACKKNIFE, _G, SKY_PLANE, "global")
MAIN = ("sky", "none-stored", "none-plane", "jk32-sliced", "jk32-global", "boot-sliced", "boot-global", "image-sliced", "image-global")
# a kernel trace tells kernels apart by name: sky_kernel, and resample_kernel<LDS_CUBE, STOKES, SKY_PLANE, IMAGE>
TRACE_GROUPS = [("sky", "none-stored", "none-plane", "jk32-global", "image-sliced"), ("jk32-sliced", "boot-global", "image-global"), ("boot-sliced",)]
_dp = C.POINTER(C.c_double)
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------- the definitions in NumPy (the read-back route)
def philox(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def block(rank, slot, number, mode):
    return philox(slot, rank, number, 2 | (mode << 8), SEED & 0xFFFFFFFF, SEED >> 32)


def host_cube(ph, clocks, rank, slot, obs, te, ee, xe, ye, mode, n_rep, frame):
    """one observer's cube [n_rep][n_t][n_e][n_y][n_x] from read-back columns, with sum|term| beside every sum"""
    n, cos_acc, ex, ey = obs
    image = xe is not None
    n_t, n_e = len(te) - 1, len(ee) - 1
    n_x, n_y = (len(xe) - 1, len(ye) - 1) if image else (1, 1)
    per_rep = n_t * n_e * n_y * n_x
    p0, p1, p2, p3, r0, r1, r2, w = (ph[k] for k in ("p0", "p1", "p2", "p3", "r0", "r1", "r2", "weight"))
    observable = (w != 0) & (ph["type"] != b"p") & (ph["type"] != b"N")
    idx = np.nonzero(observable & (((p1 * n[0, 0] + p2 * n[1, 0]) + p3 * n[2, 0]) >= p0 * cos_acc[0]))[0]
    t = clocks[idx] - (((r0[idx] * n[0, 0] + r1[idx] * n[1, 0]) + r2[idx] * n[2, 0]) / C_LIGHT)
    e = p0[idx] * C_LIGHT
    it, ie = sky_bench.find_bin(te, t), sky_bench.find_bin(ee, e)
    inside, flat = (it >= 0) & (ie >= 0), it * n_e + ie
    if image:
        ix = sky_bench.find_bin(xe, (r0[idx] * ex[0, 0] + r1[idx] * ex[1, 0]) + r2[idx] * ex[2, 0])
        iy = sky_bench.find_bin(ye, (r0[idx] * ey[0, 0] + r1[idx] * ey[1, 0]) + r2[idx] * ey[2, 0])
        inside, flat = inside & (ix >= 0) & (iy >= 0), (flat * n_y + iy) * n_x + ix
    res = {"n_accepted": len(idx), "n_outside": int((~inside).sum())}
    q, u = ph["s1"][idx], ph["s2"][idx]
    if frame == SKY_PLANE:
        a1, a2, a3 = p1[idx], p2[idx], p3[idx]
        with np.errstate(all="ignore"):
            rho2 = a1 * a1 + a2 * a2
            d = a2 * ey[0, 0] - a1 * ey[1, 0]
            s = (rho2 * ey[2, 0] - a3 * (a1 * ey[0, 0] + a2 * ey[1, 0])) / np.sqrt(rho2 + a3 * a3)
            h = np.sqrt(d * d + s * s)
            ok = (h > 0) & np.isfinite(h)
            c, sg = d / h, s / h
            c2, s2 = c * c - sg * sg, (-2.0 * sg) * c
            q, u = np.where(ok, q * c2 - u * s2, q), np.where(ok, q * s2 + u * c2, u)
        res["n_frame_undefined"] = int((~ok).sum())
    else:
        res["n_frame_undefined"] = 0
    idx, flat, e, q, u = idx[inside], flat[inside], e[inside], q[inside], u[inside]
    wi = w[idx]
    terms = {"w": wi, "we": wi * e, "i": wi * ph["s0"][idx], "q": wi * q, "u": wi * u, "v": wi * ph["s3"][idx]}
    res["count"] = np.zeros((n_rep, per_rep), dtype=np.int64)
    for k in SUMS:
        res[k], res["abs_" + k] = np.zeros((n_rep, per_rep)), np.zeros((n_rep, per_rep))
    group = ((block(rank[idx], slot[idx], 0, JACKKNIFE)[0] * np.uint64(n_rep)) >> np.uint64(32)).astype(np.int64) if mode == JACKKNIFE else None
    words = None
    for rho in range(n_rep):
        if mode == JACKKNIFE:
            mult = (group == rho).astype(np.int64)
        elif mode == BOOTSTRAP and rho >= 1:
            j = rho - 1
            if j & 3 == 0:
                words = block(rank[idx], slot[idx], j >> 2, BOOTSTRAP)
            mult = sum((words[j & 3] >= np.uint64(th)).astype(np.int64) for th in THRESHOLDS)
        else:
            mult = np.ones(len(idx), dtype=np.int64)
        res["count"][rho] = np.bincount(flat, weights=mult, minlength=per_rep).astype(np.int64)
        for k in SUMS:
            kt = mult * terms[k]
            res[k][rho] = np.bincount(flat, weights=kt, minlength=per_rep)
            res["abs_" + k][rho] = np.bincount(flat, weights=np.abs(kt), minlength=per_rep)
    return res


def child(args):
    """one process with the GPU open: the pool, the shapes, then the variants named in --child"""
    from mcrat_amd import engine, synth
    names = args.child.split(",")
    frame, ph, cfg = synth.config2(n_photons=args.photons, seed=sky_bench.SEED, nzc=args.nzc, stokes=1)
    R, lens, offs = sky_bench.layout(int(ph["p0"].size))
    pool = engine.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    pool.set_hydro(frame)
    pool.pool_create(R, int(lens.max()))
    views = [pool.pool_rank(r, r) for r in range(R)]
    recs = synth.photons_to_aos(ph, engine.PHOTON_DTYPE)
    pool.pool_set_photons(list(range(R)), [recs[int(offs[r]):int(offs[r + 1])] for r in range(R)])
    remaining = 1.0 / frame["fps"]
    pool.begin_frame(1000, 0.0, remaining)
    st = pool.run(0)
    print("frame 0: %d scatterings, %d passes" % (st.frame_scatt_cnt, st.iterations), flush=True)
    clocks = remaining + remaining * np.arange(R) / R
    cols = ["p0", "p1", "p2", "p3", "r0", "r1", "r2", "weight", "s0", "s1", "s2", "s3"]

    def columns():
        per = []
        for v in views:
            out, s = {k: np.empty(v.n) for k in cols}, engine.PhotonSoA()
            s.n = v.n
            for k in cols:
                setattr(s, k, out[k].ctypes.data_as(_dp))
            out["type"] = np.empty(v.n, dtype="S1")
            s.type = out["type"].ctypes.data_as(C.c_char_p)
            v._check(v.lib.mcrat_hip_get_photons_soa(v.ctx, C.byref(s)), "get_photons_soa")
            per.append(out)
        return {k: np.concatenate([p[k] for p in per]) for k in per[0]}, [v.n for v in views]
    cat, held = columns()
    rank = np.repeat(np.arange(R), held).astype(np.uint64)
    slot = np.concatenate([np.arange(m) for m in held]).astype(np.uint64)
    per_photon_clock = np.repeat(clocks, held)
    theta = np.arccos(np.clip(cat["p3"] / cat["p0"], -1.0, 1.0))
    axis = engine.sky_observers(0.0, 0.0, float(np.percentile(theta, 90)))
    t_axis, e_all = per_photon_clock - cat["r2"] / C_LIGHT, cat["p0"] * C_LIGHT
    t_lo, t_hi, e_lo, e_hi = np.percentile(t_axis, 1), np.percentile(t_axis, 99), np.log10(np.percentile(e_all, 1)), np.log10(np.percentile(e_all, 99))
    span = float(np.percentile(np.abs(np.concatenate([cat["r0"], cat["r1"]])), 99))
    t_of, e_of, px = (lambda m: np.linspace(t_lo, t_hi, m + 1)), (lambda m: 10.0 ** np.linspace(e_lo, e_hi, m + 1)), (lambda m: np.linspace(-span, span, m + 1))
    wide_e = np.array([0.5 * e_all[e_all > 0].min(), 2.0 * e_all.max()])
    shapes = {"d": (t_of(32), e_of(32), None, None), "f": (t_of(8), e_of(16), None, None), "e": (t_of(1), wide_e, px(36), px(36))}
    print("pool: %d lists, %d slots, %d photons read back" % (R, int(pool.n), len(rank)), flush=True)

    def run(name):
        shape, mode, n_rep, frame_, path = VARIANTS[name]
        te, ee, xe, ye = shapes[shape]
        n, cos_acc, ex, ey = axis
        if mode is None:
            return pool.pool_observe_sky(n, cos_acc, te, ee, clocks)
        if path is None:
            os.environ.pop("MCRAT_HIP_RESAMPLE_PATH", None)
        else:
            os.environ["MCRAT_HIP_RESAMPLE_PATH"] = path
        return pool.pool_observe_sky_resampled(n, cos_acc, te, ee, clocks, mode, n_rep, frame_, SEED, ex, ey, xe, ye)

    results = {}
    for name in names:
        res = results[name] = run(name)
        print("%-12s path %d: %d accepted, %d outside, %d undefined frames, %d bins of %d in use, largest count %d" %
              (name, pool.observe_sky_path() if name == "sky" else pool.observe_sky_resampled_path(), res["n_accepted"].sum(), res["n_outside"].sum(),
               int(res.get("n_frame_undefined", np.zeros(1)).sum()), int((res["count"] > 0).sum()), res["count"].size, int(res["count"].max())), flush=True)
    if "sky" in results and "none-stored" in results:
        assert np.array_equal(results["sky"]["count"], results["none-stored"]["count"][:, 0]), "NONE / AS_STORED is the sky observation"
    host_ms, host_cubes = {}, {}
    if args.host:
        t_get = sky_bench.timed(columns, args.host_reps, warm=1)
        print("read-back route, get_photons_soa of the needed columns, %d lists: %s" % (R, sky_bench.fmt(t_get)))
        for name in names:
            shape, mode, n_rep, frame_, _ = VARIANTS[name]
            if mode is None:
                continue
            te, ee, xe, ye = shapes[shape]
            key = (shape, mode, n_rep, frame_)                       # the paths of one cube share the route's cube and its time
            if key not in host_cubes:
                t0 = time.perf_counter()
                cube = host_cube(cat, per_photon_clock, rank, slot, axis, te, ee, xe, ye, mode, n_rep, frame_)
                host_cubes[key] = (cube, (time.perf_counter() - t0) * 1e3)
            want, host_ms[name] = host_cubes[key]
            got = results[name]
            assert got["n_accepted"][0] == want["n_accepted"] and got["n_outside"][0] == want["n_outside"], name
            assert got["n_frame_undefined"][0] == want["n_frame_undefined"], name
            assert np.array_equal(got["count"].reshape(want["count"].shape), want["count"]), name
            for k in SUMS:
                assert (np.abs(got[k].reshape(want[k].shape) - want[k]) <= 1e-12 * want["abs_" + k]).all(), (name, k)
            print("RESULT host variant=%s route_ms=%.3f" % (name, statistics.median(t_get) + host_ms[name]), flush=True)
        print("device cubes equal the read-back route's: counts exactly, sums to 1e-12 of the bin's sum of |terms|", flush=True)
    for name in names:
        for _ in range(3):
            run(name)
    ts = {name: [] for name in names}
    for _ in range(args.reps):
        for name in names:
            t0 = time.perf_counter()
            run(name)
            ts[name].append((time.perf_counter() - t0) * 1e3)
    for name in names:
        print("RESULT variant=%s call_ms=%.4f call_min=%.4f call_max=%.4f" % (name, statistics.median(ts[name]), min(ts[name]), max(ts[name])), flush=True)
    os.environ.pop("MCRAT_HIP_RESAMPLE_PATH", None)
    pool.close()


def kernel_name(variant):
    b = lambda v: "true" if v else "false"
    shape, mode, n_rep, frame, path = VARIANTS[variant]
    if mode is None:
        return r"sky_kernel<\s*true,\s*true,\s*false\s*>"
    return r"resample_kernel<\s*%s,\s*true,\s*%s,\s*%s\s*>" % (b(path != "global"), b(frame == SKY_PLANE), b(shape == "e"))


def start(args, names, host=False, profiler=None):
    """a fresh process of this script for some variants; nothing more is started on the GPU after one that failed"""
    timeout = shutil.which("timeout")
    cmd = ([timeout, "-k", "10", "560"] if timeout else []) + (profiler or []) + [sys.executable, os.path.abspath(__file__), "--child", ",".join(names),
           "--reps", str(args.reps), "--host-reps", str(args.host_reps), "--photons", str(args.photons), "--nzc", str(args.nzc)] + (["--host"] if host else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s\n%s\nexit %d: %s" % (r.stdout[-3000:], r.stderr[-3000:], r.returncode, " ".join(cmd)))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="(internal) measure these variants, comma-separated, in this process")
    ap.add_argument("--host", action="store_true", help="(internal) also check against and time the read-back route")
    ap.add_argument("--no-trace", action="store_true", help="call times only: no runs under rocprofv3")
    ap.add_argument("--no-sweep", action="store_true", help="without the sweep over the number of jackknife groups")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--photons", type=int, default=1_000_000)
    ap.add_argument("--nzc", type=int, default=64)
    args = ap.parse_args()
    if args.child:
        return child(args)
    calls, host, kernels = {}, {}, {}
    groups = list(TRACE_GROUPS) + ([] if args.no_sweep else [("jk%d-sliced" % G, "jk%d-global" % G) for G in SWEEP])
    batches = [(MAIN, True)] + ([] if args.no_sweep else [(tuple(n for G in SWEEP for n in ("jk%d-sliced" % G, "jk%d-global" % G)), False)])
    for names, with_host in batches:
        print("---- call times%s: %s" % (", with the read-back route" if with_host else "", " ".join(names)), flush=True)
        text = start(args, names, host=with_host)
        sys.stdout.write(text)
        for line in text.splitlines():
            f = dict(kv.split("=") for kv in line.split()[1:] if "=" in kv) if line.startswith("RESULT") else {}
            if "call_ms" in f:
                calls[f["variant"]] = (float(f["call_ms"]), float(f["call_min"]), float(f["call_max"]))
            elif "route_ms" in f:
                host[f["variant"]] = float(f["route_ms"])
    if not args.no_trace:
        if shutil.which("rocprofv3") is None:
            sys.exit("rocprofv3 is needed for the kernel times (--no-trace: call times only)")
        for names in groups:
            d = tempfile.mkdtemp(prefix="resample_trace_")
            print("---- kernel trace: %s" % " ".join(names), flush=True)
            start(args, names, profiler=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
            rows = [row for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) for row in csv.DictReader(open(f))]
            for name in names:
                hit = [row for row in rows if re.search(kernel_name(name), row["Name"])]
                if len(hit) != 1:
                    sys.exit("%d rows for %s in the kernel statistics under %s" % (len(hit), name, d))
                kernels[name] = (int(hit[0]["Calls"]), float(hit[0]["AverageNs"]) / 1e3, float(hit[0]["MinNs"]) / 1e3, float(hit[0]["MaxNs"]) / 1e3)
            shutil.rmtree(d, ignore_errors=True)
    print("---- summary")
    print("%-12s %-40s %-36s %s" % ("variant", "kernel [us]: avg (min, max, calls)", "whole call [ms]: median (min, max)", "read-back route [ms]"))
    for name, (med, lo, hi) in calls.items():
        k = kernels.get(name)
        print("%-12s %-40s %-36s %s" % (name, "%.1f (%.1f, %.1f, %d)" % (k[1], k[2], k[3], k[0]) if k else "not measured",
                                        "%.3f (%.3f, %.3f)" % (med, lo, hi), "%.1f" % host[name] if name in host else ""))


if __name__ == "__main__":
    main()
