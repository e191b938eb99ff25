"""The radiation field on the device against the read-back route, on bench.py's headline pool (cfg2: 1 048 576 cells, 1e6 photons as 1025 ragged
lists, one frame propagated), for both accumulator layouts of the global path:
    python tools/radfield_bench.py --build-variants     here, before a GPU call: libmcrat_hip_radfield_plane.so and _bin.so -- the product's objects
                                                        with radfield.hip and engine.hip recompiled under -DMCRAT_RADFIELD_BIN_MAJOR=0 / 1
    python tools/radfield_bench.py [--reps 20] [--host-reps 3] [--rounds 2] [--nzc 64] [--photons 1000000]
The second form never opens the GPU itself: it starts one fresh process per layout and round, alternating the layouts (each loads its library
through MCRAT_HIP_LIB), checks every exit status and prints what they measured:
    CELLS            one bin per hydro cell: always the global path
    SHELLS 64 x 32   beyond LDS: the global path
each as the kernel's time from HIP events (a profiling context: two events around the launch -- in the bin-major build around the launch and the
transposition) and as the whole call's time (a host clock around mcrat_hip_pool_radiation_field, which ends in a stream synchronise: memset, copy
of the edges, kernel, the six planes read back).  Beside them, once, the only route to the same planes without the entry point: mcrat_hip_get_photons_soa
of the nine needed columns list by list, mcrat_hip_lookup_cell, the boost in NumPy and np.add.at.  The device planes must equal that route's: counts
exactly, the four sums of equal-bits terms to 1e-12 of a bin's sum of |terms|, WE_comv to 1e-6 (the two boosts round differently, and p0 - v.p
cancels at Lorentz factors of a hundred).  Prints the bytes the pass reads, from the shapes (10 B per slot for flags, type and weight, 64 B more per
counted photon), over 8 TB/s as the streaming floor.  Needs nothing outside the repository."""
import argparse
import ctypes as C
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x4D435261
HBM_PEAK = 8.0e12
LAYOUTS = {"plane": 0, "bin": 1}
SUMS = ("w", "we_lab", "we_comv", "w_nscatt", "w_temp")
_dp = C.POINTER(C.c_double)


def variant_lib(layout):
    from mcrat_amd import build
    return os.path.join(build.HERE, "libmcrat_hip_radfield_%s.so" % layout)


def build_variants():
    """every translation unit but the two that see the switch is the product build's object, so the product library is built first"""
    from mcrat_amd import build
    build.build()
    cflags = [f for f in build.FLAGS if f != "-shared"] + ["-c"]
    for layout, flag in LAYOUTS.items():
        objdir = os.path.join(build.HERE, "_obj_radfield_" + layout)
        os.makedirs(objdir, exist_ok=True)
        own = {}
        for tu in ("radfield.hip", "engine.hip"):
            own[os.path.splitext(tu)[0] + ".o"] = obj = os.path.join(objdir, os.path.splitext(tu)[0] + ".o")
            subprocess.run([build.hipcc()] + cflags + ["-DMCRAT_RADFIELD_BIN_MAJOR=%d" % flag, os.path.join(build.CSRC, tu), "-o", obj], check=True)
        objs = [own.get(os.path.splitext(s)[0] + ".o", os.path.join(build.OBJDIR, os.path.splitext(s)[0] + ".o")) for s in build.SOURCES]
        subprocess.run([build.hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + ["-o", variant_lib(layout)], check=True)
        print(variant_lib(layout))


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
    return "median %9.3f ms  (min %9.3f, max %9.3f, %d)" % (statistics.median(ts), min(ts), max(ts), len(ts))


def find_bin(edges, x):
    k = np.searchsorted(edges, x, side="right") - 1
    return np.where((k >= 0) & (k < len(edges) - 1), k, -1)


def child(args):
    from mcrat_amd import engine, synth
    frame, ph, cfg = synth.config2(n_photons=args.photons, seed=SEED, nzc=args.nzc, stokes=0)
    n = int(ph["p0"].size)
    R, lens, offs = layout(n)
    pool = engine.Engine(cfg["dimensions"], cfg["geometry"], 0, profile=True)
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
    names = ("r0", "r1", "r2", "p0", "p1", "p2", "p3", "weight", "num_scatt")

    def columns():
        """mcrat_hip_get_photons_soa of the columns a radiation field reads, nothing else, list by list"""
        per = []
        for v in views:
            out, s = {k: np.empty(v.n) for k in names}, engine.PhotonSoA()
            s.n = v.n
            for k in names:
                setattr(s, k, out[k].ctypes.data_as(_dp))
            out["type"] = np.empty(v.n, dtype="S1")
            s.type = out["type"].ctypes.data_as(C.c_char_p)
            v._check(v.lib.mcrat_hip_get_photons_soa(v.ctx, C.byref(s)), "get_photons_soa")
            per.append(out)
        return {k: np.concatenate([p[k] for p in per]) for k in per[0]}
    cat = columns()
    rr = np.sqrt((cat["r0"] * cat["r0"] + cat["r1"] * cat["r1"]) + cat["r2"] * cat["r2"])
    mu = cat["r2"] / rr
    r_edges = np.linspace(np.percentile(rr, 1), np.percentile(rr, 99), 65)
    mu_edges = np.append(np.linspace(np.percentile(mu, 1), 1.0, 33)[:-1], np.nextafter(1.0, 2.0))
    modes = {"CELLS": (engine.RADFIELD_CELLS,), "SHELLS 64 x 32": (engine.RADFIELD_SHELLS, r_edges, mu_edges)}

    def host_route(shells):
        """the same planes on the host from the read-back columns: the device's look-up, the boost in NumPy, np.add.at"""
        w, typ = cat["weight"], cat["type"]
        obs = np.nonzero((w != 0) & (typ != b"p") & (typ != b"N"))[0]
        a0, a1 = np.sqrt(cat["r0"][obs] * cat["r0"][obs] + cat["r1"][obs] * cat["r1"][obs]), cat["r2"][obs]
        inside = (a0 > frame["r0_domain"][0]) & (a0 < frame["r0_domain"][1]) & (a1 > frame["r1_domain"][0]) & (a1 < frame["r1_domain"][1])
        cell = np.where(inside, pool.lookup_cell(a0, a1), -1)
        at = obs[cell >= 0]
        cell = cell[cell >= 0]
        v = synth.hydro_vector_to_cartesian(frame, cell, np.arctan2(cat["r1"][at], cat["r0"][at]))
        e_comv = synth.lorentz_boost(v, np.stack([cat[k][at] for k in ("p0", "p1", "p2", "p3")], axis=-1))[:, 0] * synth.C_LIGHT
        terms = {"w": w[at], "we_lab": w[at] * (cat["p0"][at] * synth.C_LIGHT), "we_comv": w[at] * e_comv, "w_nscatt": w[at] * cat["num_scatt"][at],
                 "w_temp": w[at] * frame["temp"][cell]}
        if shells:
            ir, imu = find_bin(r_edges, rr[at]), find_bin(mu_edges, mu[at])
            ok = (ir >= 0) & (imu >= 0)
            bins, n_bins, shape = (ir * 32 + imu)[ok], 64 * 32, (64, 32)
            terms = {k: t[ok] for k, t in terms.items()}
        else:
            bins, n_bins, shape = cell, int(frame["num_elements"]), (int(frame["num_elements"]),)
        res = {"count": np.bincount(bins, minlength=n_bins).reshape(shape), "n_observable": len(obs), "n_unlocated": len(obs) - len(at)}
        for k in SUMS:
            res[k], res["abs_" + k] = np.zeros(n_bins), np.zeros(n_bins)
            np.add.at(res[k], bins, terms[k])
            np.add.at(res["abs_" + k], bins, np.abs(terms[k]))
            res[k], res["abs_" + k] = res[k].reshape(shape), res["abs_" + k].reshape(shape)
        return res

    observable = int(((cat["weight"] != 0) & (cat["type"] != b"p") & (cat["type"] != b"N")).sum())
    pass_bytes = int(pool.n) * 10 + observable * 64
    print("pool: %d lists, %d slots, %d counted photons, %d cells; the pass reads %.1f MB: streaming floor %.1f us at 8 TB/s (derived)" %
          (R, int(pool.n), observable, frame["num_elements"], pass_bytes / 1e6, pass_bytes / HBM_PEAK * 1e6), flush=True)
    for name, a in modes.items():
        res = pool.pool_radiation_field(*a)
        print("%-15s path %d: %d located in %d of %d bins (largest count %d), %d unlocated, %d outside" %
              (name, pool.radiation_field_path(), int(res["count"].sum()), int((res["count"] > 0).sum()), res["count"].size, int(res["count"].max()),
               res["n_unlocated"], res["n_outside"]), flush=True)
        if args.host:
            want = host_route(name != "CELLS")
            assert np.array_equal(res["count"], want["count"]) and res["n_observable"] == want["n_observable"] and res["n_unlocated"] == want["n_unlocated"], name
            for k in SUMS:
                assert (np.abs(res[k] - want[k]) <= (1e-6 if k == "we_comv" else 1e-12) * want["abs_" + k]).all(), (name, k)
    if args.host:
        print("device planes equal the read-back route's: counts exactly, sums to 1e-12 (WE_comv: 1e-6) of the bin's sum of |terms|", flush=True)
    # timings: the modes in turn, round after round, so that whatever else the machine does hits both alike
    call_ms, kernel_ms = {m: [] for m in modes}, {m: [] for m in modes}
    for a in modes.values():
        for _ in range(3):
            pool.pool_radiation_field(*a)
    for _ in range(args.reps):
        for name, a in modes.items():
            t0 = time.perf_counter()
            pool.pool_radiation_field(*a)
            call_ms[name].append((time.perf_counter() - t0) * 1e3)
            kernel_ms[name].append(pool.profile_totals()[0])
    for name in modes:
        print("RESULT layout=%s mode=%s kernel_ms=%.4f kernel_min=%.4f kernel_max=%.4f call_ms=%.3f call_min=%.3f call_max=%.3f" %
              (args.child, name.replace(" ", ""), statistics.median(kernel_ms[name]), min(kernel_ms[name]), max(kernel_ms[name]),
               statistics.median(call_ms[name]), min(call_ms[name]), max(call_ms[name])), flush=True)
    if args.host:
        t_get = timed(columns, args.host_reps, warm=1)
        print("read-back route, get_photons_soa of the nine columns and type, %d lists: %s" % (R, fmt(t_get)))
        for name in modes:
            t_bin = timed(lambda: host_route(name != "CELLS"), args.host_reps, warm=1)
            print("read-back route, lookup_cell + NumPy boost + np.add.at, %-15s %s" % (name + ":", fmt(t_bin)))
            print("RESULT host mode=%s route_ms=%.3f" % (name.replace(" ", ""), statistics.median(t_get) + statistics.median(t_bin)), flush=True)
    pool.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--child", choices=tuple(LAYOUTS), default=None, help="(internal) measure in this process with the library MCRAT_HIP_LIB names")
    ap.add_argument("--host", action="store_true", help="(internal) also check against and time the read-back route")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--photons", type=int, default=1_000_000)
    ap.add_argument("--nzc", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1, help="hydro frames propagated before the measurement (0: the photons as injected)")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    if args.child:
        return child(args)
    for name in LAYOUTS:
        if not os.path.exists(variant_lib(name)):
            sys.exit("%s is missing: python tools/radfield_bench.py --build-variants first" % variant_lib(name))
    timeout = shutil.which("timeout")
    results, host = {}, {}
    for rnd in range(args.rounds):
        for name in LAYOUTS:
            with_host = rnd == 0 and name == "plane"
            cmd = ([timeout, "-k", "10", "420"] if timeout else []) + [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps),
                   "--host-reps", str(args.host_reps), "--photons", str(args.photons), "--nzc", str(args.nzc), "--frames", str(args.frames)] + (["--host"] if with_host else [])
            print("---- round %d, %s-major accumulator%s" % (rnd, name, ", with the read-back route" if with_host else ""), flush=True)
            r = subprocess.run(cmd, env=dict(os.environ, MCRAT_HIP_LIB=variant_lib(name)), capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            if r.returncode:                               # nothing more is started on the GPU after a child that failed
                sys.exit("%s\nexit %d: %s" % (r.stderr[-3000:], r.returncode, " ".join(cmd)))
            for line in r.stdout.splitlines():
                if line.startswith("RESULT layout="):
                    f = dict(kv.split("=") for kv in line.split()[1:])
                    results.setdefault((f["layout"], f["mode"]), []).append((float(f["kernel_ms"]), float(f["call_ms"])))
                elif line.startswith("RESULT host"):
                    f = dict(kv.split("=") for kv in line.split()[2:])
                    host[f["mode"]] = float(f["route_ms"])
    print("---- summary (medians per process; one value per round)")
    print("%-14s %-8s %-28s %-28s %s" % ("mode", "layout", "kernel [ms], HIP events", "whole call [ms]", "read-back route [ms]"))
    for (lay, mode), v in sorted(results.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print("%-14s %-8s %-28s %-28s %s" % (mode, lay, " ".join("%.4f" % k for k, _ in v), " ".join("%.3f" % c for _, c in v), "%.1f" % host[mode] if mode in host else ""))


if __name__ == "__main__":
    main()
