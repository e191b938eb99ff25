"""Sky observers on the device against the read-back route and against the ring observers' kernel, on bench.py's headline pool (cfg2: 1e6 photons as
1025 ragged lists, one frame propagated):
    python tools/sky_bench.py --build-variants     here, before a GPU call: the product library, and libmcrat_hip_sky_nomatch.so -- the same sources
                                                    under -DMCRAT_SKY_NO_MATCH=1 through mcrat_amd.build.build(extra_flags=..., lib=...)
    python tools/sky_bench.py [--reps 20] [--host-reps 3] [--photons 1000000] [--nzc 64]
The second form never opens the GPU itself: it starts fresh processes one at a time, checks every exit status and prints what they measured.
The shapes:
    a         1 observer on the axis x 64 t x 32 e, no image                     beyond LDS: global path
    b         8 observers at one polar angle and eight azimuths, the same axes   global path
    c         1 observer x 8 t x 1 e x 256 x 256 pixels                          global path; with the match table (product) and without (nomatch)
    d         1 observer x 32 t x 32 e, no image                                 fits LDS: both paths, forced through MCRAT_HIP_SKY_PATH
    e         1 observer x 1 t x 1 e x 36 x 36 pixels                            fits LDS: both paths
    observe-a mcrat_hip_pool_observe, the ring observers' kernel, on shape a: on the axis ring and cone accept the same photons
Call time: a host clock around mcrat_hip_pool_observe_sky, which ends in a stream synchronise (memset, copy of the inputs, kernel, the seven planes
read back); the variants in turn, round after round; median, min and max of --reps calls after three warm-up calls each.  Kernel time: the kernel's
row of rocprofv3 --kernel-trace --stats, in runs of their own (a child traces only variants whose kernels differ in name), average, min and max over
the same calls.  Beside them, once, the only route to the same cubes without the entry point: mcrat_hip_get_photons_soa of the needed columns list
by list and the definitions in NumPy with np.add.at; the device's cubes must equal that route's (counts exactly, sums to 1e-12 of a bin's sum of
|terms|).  Prints the bytes the pass reads, from the shapes, over 8 TB/s as the streaming floor.  Needs nothing outside the repository."""
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

SEED = 0x4D435261
C_LIGHT = 2.99792458e10
HBM_PEAK = 8.0e12
SUMS = (("w", None), ("we", "e"), ("i", "s0"), ("q", "s1"), ("u", "s2"), ("v", "s3"))
# variant: (shape, forced path or None); what a kernel trace tells apart is the kernel's name, so a traced child runs one variant per name
VARIANTS = {"a": ("a", None), "b": ("b", None), "c": ("c", None), "d-lds": ("d", "lds"), "d-global": ("d", "global"), "e-lds": ("e", "lds"),
            "e-global": ("e", "global"), "observe-a": ("a", None)}
TRACE_GROUPS = (("product", ("a", "d-lds", "c", "e-lds", "observe-a")), ("product", ("b", "e-global")), ("product", ("d-global",)), ("nomatch", ("c",)))
_dp = C.POINTER(C.c_double)


def variant_lib(name):
    from mcrat_amd import build
    return build.LIB if name == "product" else os.path.join(build.HERE, "libmcrat_hip_sky_%s.so" % name)


def build_variants():
    """the product library, then the same sources without the match table.  Every translation unit but the two that see the switch compiles to what
    the product build made of it, so the variant's object folder starts as a copy of the product's without those two."""
    from mcrat_amd import build
    build.build()
    objdir = os.path.join(build.HERE, "_obj_sky_nomatch")
    os.makedirs(objdir, exist_ok=True)
    for src in build.SOURCES:
        obj = os.path.splitext(src)[0] + ".o"
        if src in ("sky.hip", "engine.hip"):
            if os.path.exists(os.path.join(objdir, obj)):
                os.remove(os.path.join(objdir, obj))
        elif os.path.exists(os.path.join(build.OBJDIR, obj)):
            shutil.copy2(os.path.join(build.OBJDIR, obj), os.path.join(objdir, obj))
    print(build.build(extra_flags=["-DMCRAT_SKY_NO_MATCH=1"], lib=variant_lib("nomatch"), objdir=objdir))


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


def find_bin(edges, x):
    k = np.searchsorted(edges, x, side="right") - 1
    return np.where((k >= 0) & (k < len(edges) - 1) & (x == x), k, -1)


def host_cube(ph, clocks, n, cos_acc, ex, ey, te, ee, xe, ye, stokes):
    """the definitions of include/mcrat_hip.h in NumPy on read-back columns; the sums by np.add.at"""
    image = xe is not None
    n_obs, n_t, n_e = n.shape[1], len(te) - 1, len(ee) - 1
    n_x, n_y = (len(xe) - 1, len(ye) - 1) if image else (1, 1)
    per_obs = n_t * n_e * n_y * n_x
    p0, p1, p2, p3, r0, r1, r2, w = (ph[k] for k in ("p0", "p1", "p2", "p3", "r0", "r1", "r2", "weight"))
    observable = (w != 0) & (ph["type"] != b"p") & (ph["type"] != b"N")
    e = p0 * C_LIGHT
    ie = find_bin(ee, e)
    terms = {"w": w, "we": w * e}
    for k, col in SUMS[2:]:
        terms[k] = w * ph[col] if stokes else None
    res = {"count": np.zeros((n_obs, per_obs), dtype=np.int64), "n_accepted": np.zeros(n_obs, dtype=np.int64), "n_outside": np.zeros(n_obs, dtype=np.int64)}
    for k, _ in SUMS:
        res[k], res["abs_" + k] = np.zeros((n_obs, per_obs)), np.zeros((n_obs, per_obs))
    for o in range(n_obs):
        idx = np.nonzero(observable & (((p1 * n[0, o] + p2 * n[1, o]) + p3 * n[2, o]) >= p0 * cos_acc[o]))[0]
        t = clocks[idx] - (((r0[idx] * n[0, o] + r1[idx] * n[1, o]) + r2[idx] * n[2, o]) / C_LIGHT)
        it, je = find_bin(te, t), ie[idx]
        inside, flat = (it >= 0) & (je >= 0), it * n_e + je
        if image:
            ix = find_bin(xe, (r0[idx] * ex[0, o] + r1[idx] * ex[1, o]) + r2[idx] * ex[2, o])
            iy = find_bin(ye, (r0[idx] * ey[0, o] + r1[idx] * ey[1, o]) + r2[idx] * ey[2, o])
            inside, flat = inside & (ix >= 0) & (iy >= 0), (flat * n_y + iy) * n_x + ix
        res["n_accepted"][o], res["n_outside"][o] = len(idx), int((~inside).sum())
        flat, idx = flat[inside], idx[inside]
        np.add.at(res["count"][o], flat, 1)
        for k, _ in SUMS:
            if terms[k] is not None:
                np.add.at(res[k][o], flat, terms[k][idx])
                np.add.at(res["abs_" + k][o], flat, np.abs(terms[k][idx]))
    shape = (n_obs, n_t, n_e, n_y, n_x) if image else (n_obs, n_t, n_e)
    for k in ("count",) + tuple(k for k, _ in SUMS) + tuple("abs_" + k for k, _ in SUMS):
        res[k] = res[k].reshape(shape)
    return res


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


def child(args):
    """one process with the GPU open: the pool, the shapes, then the variants named in --child"""
    from mcrat_amd import engine, synth
    names = args.child.split(",")
    frame, ph, cfg = synth.config2(n_photons=args.photons, seed=SEED, nzc=args.nzc, stokes=args.stokes)
    n_ph = int(ph["p0"].size)
    R, lens, offs = layout(n_ph)
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
    clocks = args.frames * remaining + remaining * np.arange(R) / R          # every list its own clock, as the ranks of a run have
    slots = int(pool.n)
    cols = ["p0", "p1", "p2", "p3", "r0", "r1", "r2", "weight"] + (["s0", "s1", "s2", "s3"] if args.stokes else [])

    def columns():
        """mcrat_hip_get_photons_soa of the columns a sky observation reads, nothing else, list by list"""
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
        return {k: np.concatenate([p[k] for p in per]) for k in per[0]}
    cat = columns()
    per_photon_clock = np.repeat(clocks, lens)

    # observers and edges from the photons themselves: percentiles of the directions, the detection times, the energies and the positions
    theta = np.arccos(np.clip(cat["p3"] / cat["p0"], -1.0, 1.0))
    half = float(np.percentile(theta, 90))
    axis = engine.sky_observers(0.0, 0.0, half)
    ring8 = engine.sky_observers(np.full(8, np.percentile(theta, 50)), np.arange(8) * (np.pi / 4), np.percentile(theta, 50))
    t_axis = per_photon_clock - cat["r2"] / C_LIGHT
    e_all = cat["p0"] * C_LIGHT
    t_lo, t_hi, e_lo, e_hi = np.percentile(t_axis, 1), np.percentile(t_axis, 99), np.log10(np.percentile(e_all, 1)), np.log10(np.percentile(e_all, 99))
    span = float(np.percentile(np.abs(np.concatenate([cat["r0"], cat["r1"]])), 99))
    t_of, e_of, px = (lambda m: np.linspace(t_lo, t_hi, m + 1)), (lambda m: 10.0 ** np.linspace(e_lo, e_hi, m + 1)), (lambda m: np.linspace(-span, span, m + 1))
    wide_e = np.array([0.5 * e_all[e_all > 0].min(), 2.0 * e_all.max()])
    shapes = {"a": (axis, t_of(64), e_of(32), None, None), "b": (ring8, t_of(64), e_of(32), None, None), "c": (axis, t_of(8), wide_e, px(256), px(256)),
              "d": (axis, t_of(32), e_of(32), None, None), "e": (axis, t_of(1), wide_e, px(36), px(36))}
    observable = int(((cat["weight"] != 0) & (cat["type"] != b"p") & (cat["type"] != b"N")).sum())
    pass_bytes = slots * 10 + observable * (88 if args.stokes else 56)
    print("pool: %d lists, %d slots, %d observable photons; the pass reads %.1f MB (%.1f us at the 8 TB/s peak, derived); observe's reads %.1f MB" %
          (R, slots, observable, pass_bytes / 1e6, pass_bytes / HBM_PEAK * 1e6, (pass_bytes - 16 * observable) / 1e6), flush=True)

    def run(name):
        shape, path = VARIANTS[name]
        (n, cos_acc, ex, ey), te, ee, xe, ye = shapes[shape]
        if name == "observe-a":         # the ring that is this cone: closed at the axis, open at cos_acc
            return pool.pool_observe([1.0], [0.0], [np.nextafter(1.0, 2.0)], cos_acc, te, ee, clocks)
        if path is None:
            os.environ.pop("MCRAT_HIP_SKY_PATH", None)
        else:
            os.environ["MCRAT_HIP_SKY_PATH"] = path
        return pool.pool_observe_sky(n, cos_acc, te, ee, clocks, ex, ey, xe, ye)

    results = {}
    for name in names:
        res = results[name] = run(name)
        print("%-10s path %d: %d accepted, %d outside, %d bins of %d in use, largest count %d" %
              (name, pool.observe_path() if name == "observe-a" else pool.observe_sky_path(), res["n_accepted"].sum(), res["n_outside"].sum(),
               int((res["count"] > 0).sum()), res["count"].size, int(res["count"].max())), flush=True)
    if "a" in results and "observe-a" in results:
        assert all(np.array_equal(results["a"][k], results["observe-a"][k]) for k in ("count", "n_accepted", "n_outside")), "on the axis the cone is the ring"
        print("shape a: the cone's counts equal the ring's (mcrat_hip_pool_observe)", flush=True)
    if args.host:
        for name in names:
            if name == "observe-a":
                continue
            (n, cos_acc, ex, ey), te, ee, xe, ye = shapes[VARIANTS[name][0]]
            want = host_cube(cat, per_photon_clock, n, cos_acc, ex, ey, te, ee, xe, ye, args.stokes)
            for k in ("count", "n_accepted", "n_outside"):
                assert np.array_equal(results[name][k], want[k]), (name, k)
            for k, _ in SUMS:
                assert (np.abs(results[name][k] - want[k]) <= 1e-12 * want["abs_" + k]).all(), (name, k)
        print("device cubes equal the read-back route's: counts exactly, sums to 1e-12 of the bin's sum of |terms|", flush=True)

    # timings: the variants in turn, round after round, so that whatever else the machine does hits all of them alike
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
        print("RESULT lib=%s variant=%s call_ms=%.4f call_min=%.4f call_max=%.4f" % (args.lib, name, statistics.median(ts[name]), min(ts[name]), max(ts[name])), flush=True)
    os.environ.pop("MCRAT_HIP_SKY_PATH", None)
    if args.host:
        t_get = timed(columns, args.host_reps, warm=1)
        print("read-back route, get_photons_soa of the needed columns, %d lists: %s" % (R, fmt(t_get)))
        for shape in ("a", "b", "c"):
            (n, cos_acc, ex, ey), te, ee, xe, ye = shapes[shape]
            t_bin = timed(lambda: host_cube(cat, per_photon_clock, n, cos_acc, ex, ey, te, ee, xe, ye, args.stokes), args.host_reps, warm=1)
            print("read-back route, NumPy binning with np.add.at, shape %s: %s" % (shape, fmt(t_bin)))
            print("RESULT host shape=%s route_ms=%.3f" % (shape, statistics.median(t_get) + statistics.median(t_bin)), flush=True)
    pool.close()


def kernel_name(variant, stokes):
    """what the kernel trace calls the kernel of a variant: the template arguments tell the paths and the image apart"""
    b = lambda v: "true" if v else "false"
    shape, path = VARIANTS[variant]
    lds = path == "lds"
    if variant == "observe-a":
        return r"observe_kernel<\s*false,\s*%s\s*>" % b(stokes)
    return r"sky_kernel<\s*%s,\s*%s,\s*%s\s*>" % (b(lds), b(stokes), b(shape in ("c", "e")))


def start(args, lib, names, host=False, profiler=None):
    """a fresh process of this script for some variants with one library; nothing more is started on the GPU after one that failed"""
    timeout = shutil.which("timeout")
    cmd = ([timeout, "-k", "10", "560"] if timeout else []) + (profiler or []) + [sys.executable, os.path.abspath(__file__), "--child", ",".join(names), "--lib", lib,
           "--reps", str(args.reps), "--host-reps", str(args.host_reps), "--photons", str(args.photons), "--nzc", str(args.nzc), "--stokes", str(args.stokes),
           "--frames", str(args.frames)] + (["--host"] if host else [])
    r = subprocess.run(cmd, env=dict(os.environ, MCRAT_HIP_LIB=variant_lib(lib)), capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s\n%s\nexit %d: %s" % (r.stdout[-3000:], r.stderr[-3000:], r.returncode, " ".join(cmd)))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--child", default=None, help="(internal) measure these variants, comma-separated, in this process with the library MCRAT_HIP_LIB names")
    ap.add_argument("--lib", default="product", help="(internal) the library's name in the output")
    ap.add_argument("--host", action="store_true", help="(internal) also check against and time the read-back route")
    ap.add_argument("--no-trace", action="store_true", help="call times only: no runs under rocprofv3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--photons", type=int, default=1_000_000)
    ap.add_argument("--nzc", type=int, default=64)
    ap.add_argument("--stokes", type=int, default=1)
    ap.add_argument("--frames", type=int, default=1, help="hydro frames propagated before the observation (0: the photons as injected)")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    if args.child:
        return child(args)
    if not os.path.exists(variant_lib("nomatch")):
        sys.exit("%s is missing: python tools/sky_bench.py --build-variants first" % variant_lib("nomatch"))
    calls, host, kernels = {}, {}, {}
    for lib, names, with_host in (("product", tuple(VARIANTS), True), ("nomatch", ("c", "a"), False)):
        print("---- call times, %s library%s" % (lib, ", with the read-back route" if with_host else ""), flush=True)
        text = start(args, lib, names, host=with_host)
        sys.stdout.write(text)
        for line in text.splitlines():
            f = dict(kv.split("=") for kv in line.split()[1:] if "=" in kv) if line.startswith("RESULT") else {}
            if "variant" in f:
                calls[(f["lib"], f["variant"])] = (float(f["call_ms"]), float(f["call_min"]), float(f["call_max"]))
            elif "shape" in f:
                host[f["shape"]] = float(f["route_ms"])
    if not args.no_trace:
        if shutil.which("rocprofv3") is None:
            sys.exit("rocprofv3 is needed for the kernel times (--no-trace: call times only)")
        for lib, names in TRACE_GROUPS:
            d = tempfile.mkdtemp(prefix="sky_trace_")
            print("---- kernel trace, %s library: %s" % (lib, " ".join(names)), flush=True)
            start(args, lib, names, profiler=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
            rows = [row for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) for row in csv.DictReader(open(f))]
            for name in names:
                hit = [row for row in rows if re.search(kernel_name(name, args.stokes), row["Name"])]
                if len(hit) != 1:
                    sys.exit("%d rows for %s in the kernel statistics under %s" % (len(hit), name, d))
                kernels[(lib, name)] = (int(hit[0]["Calls"]), float(hit[0]["AverageNs"]) / 1e3, float(hit[0]["MinNs"]) / 1e3, float(hit[0]["MaxNs"]) / 1e3)
            shutil.rmtree(d, ignore_errors=True)
    print("---- summary")
    print("%-10s %-8s %-38s %-34s %s" % ("variant", "library", "kernel [us]: avg (min, max, calls)", "whole call [ms]: median (min, max)", "read-back route [ms]"))
    for (lib, name), (med, lo, hi) in calls.items():
        k = kernels.get((lib, name))
        print("%-10s %-8s %-38s %-34s %s" % (name, lib, "%.1f (%.1f, %.1f, %d)" % (k[1], k[2], k[3], k[0]) if k else "not measured",
                                            "%.3f (%.3f, %.3f)" % (med, lo, hi), "%.1f" % host[name] if name in host else ""))


if __name__ == "__main__":
    main()
