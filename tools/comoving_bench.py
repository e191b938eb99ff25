"""The comoving radiation field on the device against the read-back route, on bench.py's headline pool (cfg2: 1 048 576 cells, 1e6 photons as 1025
ragged lists, one frame propagated):
    python tools/comoving_bench.py [--reps 20] [--host-reps 2] [--rounds 2] [--nzc 64] [--photons 1000000]
It never opens the GPU itself: it starts one fresh process per round, checks every exit status and prints what they measured:
    radiation_field SHELLS 64 x 32      the yardstick: the unchanged kernel of the radiation field on the same photons and shells, in the same run
    SHELLS 64 x 32 x 1 x 1              the same shells with one energy and one cosine bin: radfield's per-photon work plus one division, one square
                                        root and two more adds; 128 KiB of planes: the global path
    SHELLS 8 x 4 x 32 x 8               spectra and beaming per shell: 8192 bins, the global path
    SHELLS 8 x 4 x 1 x 8                256 bins: the LDS path by the rule, and the global path under MCRAT_HIP_COMOVING_PATH=global
    CELLS x 1 x 8                       eight cosine bins per hydro cell: 8.4 million bins, 512 MiB of planes
each as the kernel's time from HIP events (a profiling context: two events around the launch) and as the whole call's time (a host clock around
mcrat_hip_pool_comoving_field, which ends in a stream synchronise: memset, copy of the edges, kernel, the eight planes read back).  Beside them,
once, the only route to the same planes without the entry point: mcrat_hip_get_photons_soa of the eight needed columns list by list,
mcrat_hip_lookup_cell, the boost in NumPy and np.add.at.  The device planes must equal that route's: n_observable and n_unlocated exactly, counts but
for the handful of photons within rounding of an energy or cosine edge (at most 8 in a million, printed), sums to 1e-6 of a bin's sum of |w e| (|w| for w) in
the bins whose counts agree.  Needs nothing outside the repository."""
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
SUMS = ("w", "we", "wea", "weaa", "we_lab", "wem", "wemm")
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


def timed(fn, reps, warm=1):
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
    return np.where((k >= 0) & (k < len(edges) - 1) & (x == x), k, -1)


def clamp(x):
    return np.where(x < -1.0, -1.0, np.where(x > 1.0, 1.0, x))


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
    names = ("r0", "r1", "r2", "p0", "p1", "p2", "p3", "weight")

    def columns():
        """mcrat_hip_get_photons_soa of the columns a comoving field reads, nothing else, list by list"""
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

    def per_photon():
        """the located photons' quantities on the host from the read-back columns: the device's look-up, the textbook boost in NumPy"""
        w, typ = cat["weight"], cat["type"]
        obs = np.nonzero((w != 0) & (typ != b"p") & (typ != b"N"))[0]
        a0, a1 = np.sqrt(cat["r0"][obs] * cat["r0"][obs] + cat["r1"][obs] * cat["r1"][obs]), cat["r2"][obs]
        inside = (a0 > frame["r0_domain"][0]) & (a0 < frame["r0_domain"][1]) & (a1 > frame["r1_domain"][0]) & (a1 < frame["r1_domain"][1])
        cell = np.where(inside, pool.lookup_cell(a0, a1), -1)
        at = obs[cell >= 0]
        cell = cell[cell >= 0]
        r0, r1, r2 = (cat[k][at] for k in ("r0", "r1", "r2"))
        p = [cat[k][at] for k in ("p0", "p1", "p2", "p3")]
        v = synth.hydro_vector_to_cartesian(frame, cell, np.arctan2(r1, r0))
        pp = synth.lorentz_boost(v, np.stack(p, axis=-1))
        b = np.sqrt((v * v).sum(axis=1))
        rr = np.sqrt((r0 * r0 + r1 * r1) + r2 * r2)
        m = clamp(((p[1] * r0 + p[2] * r1) + p[3] * r2) / (p[0] * rr))
        with np.errstate(invalid="ignore", divide="ignore"):
            a = np.where(b > 0, clamp((pp[:, 1:] * v).sum(axis=1) / (b * pp[:, 0])), m)
        we, wl = w[at] * (pp[:, 0] * synth.C_LIGHT), w[at] * (p[0] * synth.C_LIGHT)
        return dict(n_observable=len(obs), n_unlocated=len(obs) - len(at), cell=cell, r=rr, mu=r2 / rr, e=pp[:, 0] * synth.C_LIGHT, a=a,
                    terms={"w": w[at], "we": we, "wea": we * a, "weaa": we * a * a, "we_lab": wl, "wem": wl * m, "wemm": wl * m * m})
    q = per_photon()
    r64 = np.linspace(np.percentile(q["r"], 1), np.percentile(q["r"], 99), 65)
    mu32 = np.append(np.linspace(np.percentile(q["mu"], 1), 1.0, 33)[:-1], np.nextafter(1.0, 2.0))
    r8, mu4 = r64[::8].copy(), mu32[::8].copy()
    e32 = 10.0 ** np.linspace(np.log10(np.percentile(q["e"], 1)), np.log10(np.percentile(q["e"], 99)), 33)
    e1, a1, a8 = np.array([0.0, 1e300]), np.array([-1.0, 2.0]), engine.cosine_edges(8)
    S, CL = engine.COMOVING_SHELLS, engine.COMOVING_CELLS
    # name: (forced path or None, the arguments of pool_comoving_field)
    shapes = {"SHELLS 64x32x1x1": (None, (S, e1, a1, r64, mu32)), "SHELLS 8x4x32x8": (None, (S, e32, a8, r8, mu4)),
              "SHELLS 8x4x1x8 lds": (None, (S, e1, a8, r8, mu4)), "SHELLS 8x4x1x8 global": ("global", (S, e1, a8, r8, mu4)),
              "CELLS x1x8": (None, (CL, e1, a8))}

    def run(name):
        if name == "radiation_field SHELLS 64x32":
            return pool.pool_radiation_field(engine.RADFIELD_SHELLS, r64, mu32)
        forced, a = shapes[name]
        if forced:
            os.environ["MCRAT_HIP_COMOVING_PATH"] = forced
        try:
            return pool.pool_comoving_field(*a)
        finally:
            os.environ.pop("MCRAT_HIP_COMOVING_PATH", None)

    def host_route(name):
        """the same planes on the host: bins from the per-photon quantities, np.add.at"""
        mode, e_edges, a_edges = shapes[name][1][:3]
        if mode == S:
            r_edges, mu_edges = shapes[name][1][3:]
            ir, imu = find_bin(r_edges, q["r"]), find_bin(mu_edges, q["mu"])
            s, n_s = np.where((ir >= 0) & (imu >= 0), ir * (len(mu_edges) - 1) + imu, -1), (len(r_edges) - 1) * (len(mu_edges) - 1)
        else:
            s, n_s = q["cell"], int(frame["num_elements"])
        n_e, n_a = len(e_edges) - 1, len(a_edges) - 1
        ie, ia = find_bin(e_edges, q["e"]), find_bin(a_edges, q["a"])
        ok = (s >= 0) & (ie >= 0) & (ia >= 0)
        bins, n_bins = ((s * n_e + ie) * n_a + ia)[ok], n_s * n_e * n_a
        res = {"count": np.bincount(bins, minlength=n_bins), "n_observable": q["n_observable"], "n_unlocated": q["n_unlocated"]}
        for k in SUMS:
            res[k], res["abs_" + k] = np.zeros(n_bins), np.zeros(n_bins)
            np.add.at(res[k], bins, q["terms"][k][ok])
            np.add.at(res["abs_" + k], bins, np.abs(q["terms"][k][ok]))
        return res

    print("pool: %d lists, %d slots, %d counted photons, %d cells" % (R, int(pool.n), q["n_observable"], frame["num_elements"]), flush=True)
    order = ["radiation_field SHELLS 64x32"] + list(shapes)
    for name in order:
        res = run(name)
        path = pool.radiation_field_path() if name.startswith("radiation") else pool.comoving_field_path()
        print("%-30s path %d: %d located in %d of %d bins (largest count %d), %d unlocated, %d outside" %
              (name, path, int(res["count"].sum()), int((res["count"] > 0).sum()), res["count"].size, int(res["count"].max()), res["n_unlocated"],
               res["n_outside"]), flush=True)
        if name == "SHELLS 8x4x32x8":
            mom = engine.eddington_moments(res)
            used = mom["J"] > 0
            print("    K / J in the fluid frame: median %.3f (min %.3f, max %.3f); in the lab about the radial direction: median %.4f" %
                  (np.median(mom["K_over_J"][used]), mom["K_over_J"][used].min(), mom["K_over_J"][used].max(), np.median(mom["K_over_J_lab"][used])), flush=True)
        if args.host and name in shapes:
            want = host_route(name)
            assert res["n_observable"] == want["n_observable"] and res["n_unlocated"] == want["n_unlocated"], name
            same = res["count"].ravel() == want["count"]
            moved = int(np.abs(res["count"].ravel() - want["count"]).sum())
            print("    against the read-back route: %d counts differ in all (photons within rounding of an edge)" % moved, flush=True)
            assert moved <= 16, name                       # a photon that changes its bin changes two counts
            for k in SUMS:                                 # (the planes with a or m in them on the scale of their energy plane: a may be 0)
                scale = want["abs_we"] if k in ("wea", "weaa") else want["abs_we_lab"] if k in ("wem", "wemm") else want["abs_" + k]
                assert (np.abs(res[k].ravel() - want[k]) <= 1e-6 * scale)[same].all(), (name, k)
    if args.host:
        print("device planes equal the read-back route's: sums to 1e-6 of the bin's sum of |w e| (|w| for w)", flush=True)
    # timings: the shapes in turn, round after round, so that whatever else the machine does hits all alike
    call_ms, kernel_ms = {m: [] for m in order}, {m: [] for m in order}
    for name in order:
        for _ in range(2):
            run(name)
    for _ in range(args.reps):
        for name in order:
            t0 = time.perf_counter()
            run(name)
            call_ms[name].append((time.perf_counter() - t0) * 1e3)
            kernel_ms[name].append(pool.profile_totals()[0])
    for name in order:
        print("RESULT shape=%s kernel_ms=%.4f kernel_min=%.4f kernel_max=%.4f call_ms=%.3f call_min=%.3f call_max=%.3f" %
              (name.replace(" ", "_"), statistics.median(kernel_ms[name]), min(kernel_ms[name]), max(kernel_ms[name]),
               statistics.median(call_ms[name]), min(call_ms[name]), max(call_ms[name])), flush=True)
    if args.host:
        t_get = timed(columns, args.host_reps)
        print("read-back route, get_photons_soa of the eight columns and type, %d lists: %s" % (R, fmt(t_get)))
        t_ph = timed(per_photon, args.host_reps)
        print("read-back route, lookup_cell + NumPy boost and cosines:                    %s" % fmt(t_ph))
        for name in shapes:
            if name.endswith("global"):
                continue
            t_bin = timed(lambda: host_route(name), args.host_reps)
            print("read-back route, the bins and np.add.at of seven planes, %-20s %s" % (name + ":", fmt(t_bin)))
            print("RESULT host shape=%s route_ms=%.3f" % (name.replace(" ", "_"), statistics.median(t_get) + statistics.median(t_ph) + statistics.median(t_bin)), flush=True)
    pool.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    ap.add_argument("--host", action="store_true", help="(internal) also check against and time the read-back route")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--photons", type=int, default=1_000_000)
    ap.add_argument("--nzc", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1, help="hydro frames propagated before the measurement (0: the photons as injected)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    timeout = shutil.which("timeout")
    results, host = {}, {}
    for rnd in range(args.rounds):
        with_host = rnd == 0
        cmd = ([timeout, "-k", "10", "540"] if timeout else []) + [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
               "--host-reps", str(args.host_reps), "--photons", str(args.photons), "--nzc", str(args.nzc), "--frames", str(args.frames)] + (["--host"] if with_host else [])
        print("---- round %d%s" % (rnd, ", with the read-back route" if with_host else ""), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode:                               # nothing more is started on the GPU after a child that failed
            sys.exit("%s\nexit %d: %s" % (r.stderr[-3000:], r.returncode, " ".join(cmd)))
        for line in r.stdout.splitlines():
            if line.startswith("RESULT shape="):
                f = dict(kv.split("=") for kv in line.split()[1:])
                results.setdefault(f["shape"], []).append((float(f["kernel_ms"]), float(f["call_ms"])))
            elif line.startswith("RESULT host"):
                f = dict(kv.split("=") for kv in line.split()[2:])
                host[f["shape"]] = float(f["route_ms"])
    print("---- summary (medians per process; one value per round)")
    print("%-32s %-28s %-28s %s" % ("shape", "kernel [ms], HIP events", "whole call [ms]", "read-back route [ms]"))
    for shape, v in results.items():
        print("%-32s %-28s %-28s %s" % (shape, " ".join("%.4f" % k for k, _ in v), " ".join("%.3f" % c for _, c in v), "%.1f" % host[shape] if shape in host else ""))
    yard, one = results.get("radiation_field_SHELLS_64x32"), results.get("SHELLS_64x32x1x1")
    if yard and one:
        print("yardstick: comoving_field SHELLS 64x32x1x1 / radiation_field SHELLS 64x32, kernel: %s" %
              " ".join("%.2f" % (o[0] / y[0]) for o, y in zip(one, yard)))


if __name__ == "__main__":
    main()
