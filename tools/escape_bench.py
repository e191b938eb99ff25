"""Escape-weighted sky observations on the device against the routes the other products offer, on bench.py's headline pool (cfg2: 1e6 photons as
1025 ragged lists on the synth frame, one frame propagated):
    python tools/escape_bench.py [--reps 10] [--host-reps 2] [--photons 1000000] [--nzc 64] [--frames 1]
It never opens the GPU itself: it starts one fresh process under a time limit, checks its exit status and prints what it measured.
The shapes, each one observer on the polar axis with six optical-depth bins (0, 0.1, 0.3, 1, 3, 10, 30):
    lc2       a light curve, 64 t x 1 e, with a cone of 2 degrees            fits LDS: both paths, forced through MCRAT_HIP_ESCAPE_PATH
    lc30      the same with a cone of 30 degrees                             both paths
    img       one image, 1 t x 1 e x 128 x 128 pixels, cone of 30 degrees    beyond LDS: the global path
Side by side, per shape:
    (a) mcrat_hip_pool_observe_escaping, the new call;
    (b) the route without it: mcrat_hip_pool_sightline_photons over all slots with tau and status read back, mcrat_hip_get_photons_soa of the columns
        the binning needs, then NumPy binning by tests/sky_checker.py's rules with np.add.at;
    (c) mcrat_hip_pool_sightline_photons alone;
    (d) mcrat_hip_pool_observe_sky alone.
Call time: a host clock around the call, which ends in a stream synchronise; the variants in turn, round after round; median, min and max of --reps
calls after two warm-up calls each.  The device's cube must equal route (b)'s: counts exactly, sums to 1e-12 of a bin's sum of |terms| (WX, WEX:
1e-9, the two exp).  Prints n_selected / n_observable for each shape.  Needs nothing outside the repository."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sky_bench                                     # noqa: E402  (bench.py's list layout, the timing helpers)

C_LIGHT = 2.99792458e10
TAU_EDGES = np.array([0.0, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0])
MARCH = dict(step_frac=0.01, h_min=1e6, max_steps=1024)          # tools/sightline_bench.py's cfg2 workload
LEFT_MESH = 1
SUMS = ("w", "we", "i", "q", "u", "v", "wx", "wex")
_dp = C.POINTER(C.c_double)


def host_cube(ph, clocks, tau, status, n, cos_acc, ex, ey, te, ee, xe, ye, stokes):
    """the definitions of include/mcrat_hip.h in NumPy on read-back columns, tau and status; the sums by np.add.at"""
    image = xe is not None
    n_tau, n_t, n_e = len(TAU_EDGES) - 1, len(te) - 1, len(ee) - 1
    n_x, n_y = (len(xe) - 1, len(ye) - 1) if image else (1, 1)
    per_obs = n_tau * n_t * n_e * n_y * n_x
    p0, p1, p2, p3, r0, r1, r2, w = (ph[k] for k in ("p0", "p1", "p2", "p3", "r0", "r1", "r2", "weight"))
    observable = (w != 0) & (ph["type"] != b"p") & (ph["type"] != b"N")
    e = p0 * C_LIGHT
    x = np.exp(-tau)
    terms = {"w": w, "we": w * e, "wx": w * x, "wex": (w * e) * x}
    for k, col in (("i", "s0"), ("q", "s1"), ("u", "s2"), ("v", "s3")):
        terms[k] = w * ph[col] if stokes else None
    res = {"count": np.zeros(per_obs, dtype=np.int64)}
    for k in SUMS:
        res[k], res["abs_" + k] = np.zeros(per_obs), np.zeros(per_obs)
    idx = np.nonzero(observable & (((p1 * n[0, 0] + p2 * n[1, 0]) + p3 * n[2, 0]) >= p0 * cos_acc[0]))[0]
    res["n_accepted"] = len(idx)
    idx = idx[status[idx] == LEFT_MESH]
    t = clocks[idx] - (((r0[idx] * n[0, 0] + r1[idx] * n[1, 0]) + r2[idx] * n[2, 0]) / C_LIGHT)
    itau, it, ie = sky_bench.find_bin(TAU_EDGES, tau[idx]), sky_bench.find_bin(te, t), sky_bench.find_bin(ee, e[idx])
    inside, flat = (itau >= 0) & (it >= 0) & (ie >= 0), (itau * n_t + it) * n_e + ie
    if image:
        ix = sky_bench.find_bin(xe, (r0[idx] * ex[0, 0] + r1[idx] * ex[1, 0]) + r2[idx] * ex[2, 0])
        iy = sky_bench.find_bin(ye, (r0[idx] * ey[0, 0] + r1[idx] * ey[1, 0]) + r2[idx] * ey[2, 0])
        inside, flat = inside & (ix >= 0) & (iy >= 0), (flat * n_y + iy) * n_x + ix
    flat, idx = flat[inside], idx[inside]
    np.add.at(res["count"], flat, 1)
    for k in SUMS:
        if terms[k] is not None:
            np.add.at(res[k], flat, terms[k][idx])
            np.add.at(res["abs_" + k], flat, np.abs(terms[k][idx]))
    return res


def child(args):
    """one process with the GPU open: the pool, the shapes, the four routes"""
    from mcrat_amd import engine, synth
    frame, ph, cfg = synth.config2(n_photons=args.photons, seed=sky_bench.SEED, nzc=args.nzc, stokes=args.stokes)
    R, lens, offs = sky_bench.layout(int(ph["p0"].size))
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
    clocks = args.frames * remaining + remaining * np.arange(R) / R
    slots = int(pool.n)
    stride = slots // R
    cols = ["p0", "p1", "p2", "p3", "r0", "r1", "r2", "weight"] + (["s0", "s1", "s2", "s3"] if args.stokes else [])

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
        return {k: np.concatenate([p[k] for p in per]) for k in per[0]}
    cat = columns()
    per_photon_clock = np.repeat(clocks, lens)
    in_list = np.concatenate([r * stride + np.arange(lens[r]) for r in range(R)])        # the pool's slots that belong to a list, list by list

    t_axis = per_photon_clock - cat["r2"] / C_LIGHT
    e_all = cat["p0"] * C_LIGHT
    span = float(np.percentile(np.abs(np.concatenate([cat["r0"], cat["r1"]])), 99))
    te64, te1 = np.linspace(np.percentile(t_axis, 1), np.percentile(t_axis, 99), 65), np.array([t_axis.min() - 1.0, t_axis.max() + 1.0])
    wide_e = np.array([0.5 * e_all[e_all > 0].min(), 2.0 * e_all.max()])
    px = np.linspace(-span, span, 129)
    shapes = {"lc2": (engine.sky_observers(0.0, 0.0, np.radians(2.0)), te64, wide_e, None, None),
              "lc30": (engine.sky_observers(0.0, 0.0, np.radians(30.0)), te64, wide_e, None, None),
              "img": (engine.sky_observers(0.0, 0.0, np.radians(30.0)), te1, wide_e, px, px)}

    def escaping(shape, path):
        (n, cos_acc, ex, ey), te, ee, xe, ye = shapes[shape]
        if path is None:
            os.environ.pop("MCRAT_HIP_ESCAPE_PATH", None)
        else:
            os.environ["MCRAT_HIP_ESCAPE_PATH"] = path
        return pool.pool_observe_escaping(n, cos_acc, te, ee, TAU_EDGES, clocks, ex=ex, ey=ey, x_edges=xe, y_edges=ye, **MARCH)

    def sightlines():
        return pool.pool_sightline_photons(**MARCH)

    def sky(shape):
        (n, cos_acc, ex, ey), te, ee, xe, ye = shapes[shape]
        return pool.pool_observe_sky(n, cos_acc, te, ee, clocks, ex, ey, xe, ye)

    def route_b(shape):
        (n, cos_acc, ex, ey), te, ee, xe, ye = shapes[shape]
        sl = sightlines()
        ph_now = columns()
        return host_cube(ph_now, per_photon_clock, sl["tau"][in_list], sl["status"][in_list], n, cos_acc, ex, ey, te, ee, xe, ye, args.stokes)

    variants = {}
    for shape in shapes:
        for path in (("lds", "global") if shape != "img" else (None,)):
            variants["%s-%s" % (shape, path or "rule")] = (lambda shape=shape, path=path: escaping(shape, path))
        variants["%s-sky" % shape] = (lambda shape=shape: sky(shape))
    variants["sightlines"] = sightlines

    for shape in shapes:
        res = escaping(shape, None)
        want = route_b(shape)
        print("%-5s path %d: n_selected / n_observable = %d / %d = %.4f; accepted %d, in bins %d, outside %d, opaque %d, unresolved %d; n_status %s" %
              (shape, pool.observe_escaping_path(), res["n_selected"], res["n_observable"], res["n_selected"] / max(res["n_observable"], 1), res["n_accepted"][0],
               int(res["count"].sum()), res["n_outside"][0], res["n_opaque"][0], res["n_unresolved"][0], res["n_status"].tolist()), flush=True)
        assert res["n_accepted"][0] == want["n_accepted"] and np.array_equal(res["count"].ravel(), want["count"]), shape
        for k in SUMS:
            tol = 1e-9 if k in ("wx", "wex") else 1e-12
            assert (np.abs(res[k].ravel() - want[k]) <= tol * want["abs_" + k]).all(), (shape, k)
        frac = engine.escape_fraction(res)
        print("      escape fraction WX / W per tau bin: %s" % np.array2string(np.nansum(res["wx"], axis=tuple(range(2, res["wx"].ndim)))[0] /
                                                                                 np.maximum(np.nansum(res["w"], axis=tuple(range(2, res["w"].ndim)))[0], 1e-300), precision=4),
              "(bins in use: %d)" % int(np.isfinite(frac).sum()), flush=True)
    print("device cubes equal route (b)'s: counts exactly, sums to 1e-12 (WX, WEX 1e-9) of the bin's sum of |terms|", flush=True)

    for fn in variants.values():
        for _ in range(2):
            fn()
    ts = {name: [] for name in variants}
    for _ in range(args.reps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    os.environ.pop("MCRAT_HIP_ESCAPE_PATH", None)
    for name in variants:
        print("RESULT variant=%s call_ms=%.4f call_min=%.4f call_max=%.4f" % (name, statistics.median(ts[name]), min(ts[name]), max(ts[name])), flush=True)
    for shape in shapes:
        t = sky_bench.timed(lambda: route_b(shape), args.host_reps, warm=1)
        print("RESULT variant=%s-route-b call_ms=%.4f call_min=%.4f call_max=%.4f" % (shape, statistics.median(t), min(t), max(t)), flush=True)
    pool.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--photons", type=int, default=1_000_000)
    ap.add_argument("--nzc", type=int, default=64)
    ap.add_argument("--stokes", type=int, default=1)
    ap.add_argument("--frames", type=int, default=1, help="hydro frames propagated before the observation (0: the photons as injected)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    timeout = shutil.which("timeout")
    cmd = ([timeout, "-k", "10", "540"] if timeout else []) + [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--host-reps",
           str(args.host_reps), "--photons", str(args.photons), "--nzc", str(args.nzc), "--stokes", str(args.stokes), "--frames", str(args.frames)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode:
        sys.exit("%s\nexit %d: %s" % (r.stderr[-3000:], r.returncode, " ".join(cmd)))
    calls = {}
    for line in r.stdout.splitlines():
        if line.startswith("RESULT"):
            f = dict(kv.split("=") for kv in line.split()[1:])
            calls[f["variant"]] = (float(f["call_ms"]), float(f["call_min"]), float(f["call_max"]))
    show = lambda k: "%9.3f (%8.3f, %8.3f)" % calls[k] if k in calls else "       --"
    print("---- summary: whole calls [ms], median (min, max)")
    print("%-6s %-30s %-30s %-30s %-30s %-30s" % ("shape", "(a) escaping, lds", "(a) escaping, global", "(b) sightlines+read-back+NumPy", "(c) sightlines alone", "(d) observe_sky alone"))
    for shape in ("lc2", "lc30", "img"):
        print("%-6s %-30s %-30s %-30s %-30s %-30s" % (shape, show(shape + "-lds"), show(shape + "-global") if shape != "img" else show("img-rule"), show(shape + "-route-b"),
                                                      show("sightlines"), show(shape + "-sky")))


if __name__ == "__main__":
    main()
