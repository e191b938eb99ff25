"""An independent NumPy restatement of the comoving radiation field (include/mcrat_hip.h) on a synth frame dict, for
tests/test_gpu_comoving.py and tests/test_comoving_checker_cpu.py, built on tests/radfield_checker.py (the counted slots, r, mu, the cell by brute
force, e_lab, the fluid-frame energy from synth.lorentz_boost and its bar) and tests/sightline_checker.py (locate).  Not a copy of the kernel:

  * the cell's velocity v from synth.hydro_vector_to_cartesian at arctan2(r1, r0);
  * a = (p' . v_hat) / p'0 with p' the textbook boost of synth.lorentz_boost, which takes its Lorentz factor from |v| -- not the closed form the
    device evaluates; a cell at rest: a = m;
  * m in the definition's exact expression, so that it and the lab terms w*e_lab, (w*e_lab)*m, ((w*e_lab)*m)*m are the same bits on both sides.

How far a device sum may lie from the checker's, per bin with n terms t_i, u = 2^-53:

  w, we_lab, wem, wemm   (n + 2) u sum|t_i|: the worst case of adding n equal-bits terms in any order, plus room for the final roundings.
  we                     sum 2 bar_e,i |t_i| + (n + 2) u sum|t_i|, bar_e = 8u (1 + |x_v|)(1 + Gamma_v^2) / (1 - x_v), x_v = v.p / p0: radfield_checker's.
  wea, weaa              a conditioning bar for a on top.  Write x = v.p / p0 = b cos(theta), b = |v|; then a = N / D with N / p0 = x / b - b and
                         D / p0 = 1 - x.  Let eta = 8u stand for what one side's operands carry, as in bar_e: the components of v (an azimuth's
                         cosine and sine times the staged record on the device, cos and sin of arctan2 here) and the roundings of a three-term dot
                         product.  The products of v.p are bounded by b p0, so x carries an ABSOLUTE error eta b -- relative to 1 - x that is the
                         amplification b / (1 - x) -- and b a relative one of eta.  Then
                             d(x / b) <= d(x) / b + |x / b| d(b) / b <= eta (1 + |cos theta|) <= 2 eta
                             d(N / p0) <= 2 eta + eta b <= 3 eta             (absolute: N cancels where a ~ 0, its error does not)
                             d(D / p0) <= eta b
                             d(a) <= (d(N / p0) + |a| d(D / p0)) / (1 - x) <= eta (3 + |a| b) / (1 - x)  =: bar_a
                         Since 1 / (1 - x) <= 1 / (1 - b) = Gamma_v^2 (1 + b), bar_a <= 64 u Gamma_v^2: the absolute error of a scales like
                         u (1 + Gamma_v^2).  The textbook boost here sums terms of size Gamma p0 into p' . v_hat = Gamma N and divides by p'0 = Gamma D:
                         its Lorentz factor cancels to first order and its roundings are a few u / (1 - x), inside bar_a.  Clamping into
                         [-1, 1] moves both sides towards each other or not at all.  Taken twice because both sides round, d = 2 bar_a:
                             wea    sum (2 bar_e |a| + d) |w e|            + (n + 2) u sum|t_i|
                             weaa   sum (2 bar_e a^2 + 2 |a| d + d^2) |w e| + (n + 2) u sum|t_i|
                         Derived, not tuned.  The largest bar_a on the committed cases is 4.4e-13 for gamma <= 10 and 2.9e-13 in the case with
                         gamma <= 100 (whose photons head mostly outwards, not along the random flows); on 20 000 photons of which a tenth
                         are sent within 0.02 rad of the flow it is 6.7e-13 and 1.3e-11, and the closed form the device evaluates lies within
                         0.31 bar_a of the textbook boost (tests/test_comoving_checker_cpu.py asserts these figures).

and which photons it cannot judge: `fragile`, a counted, located photon that locate marks near a face (radfield_checker's rule), or whose e bin
differs between e (1 - 2 bar_e) and e (1 + 2 bar_e), or whose a bin differs between a - 2 bar_a and a + 2 bar_a, both clamped into [-1, 1] as a
itself is -- a photon within its bar of an edge.  The committed cases below hold none (tests/test_comoving_checker_cpu.py asserts it), so the window
the GPU comparison grants for them -- per bin, the count without the fragile photons up to that count plus their number -- is of width zero."""
import functools

import numpy as np

from mcrat_amd import synth
from tests import radfield_checker as rc
from tests.sightline_checker import PAIRS, mesh, random_fluid

CELLS, SHELLS = 0, 1
U = 2.0 ** -53
SUMS = ("w", "we", "wea", "weaa", "we_lab", "wem", "wemm")
find_bin = rc.find_bin


def clamp(x):
    """into [-1, 1]; a NaN stays a NaN"""
    return np.where(x < -1.0, -1.0, np.where(x > 1.0, 1.0, x))


def cosines(v, p, r):
    """v (n, 3), p (4, n), r (3, n) -> (m, a, bar_a): the lab cosine about the radial direction in the definition's expression, the fluid-frame cosine
    about the flow from the textbook boost (m where v == 0), and a's conditioning bar (0 where v == 0: a is m, the same bits)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        rr = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        m = clamp(((p[1] * r[0] + p[2] * r[1]) + p[3] * r[2]) / (p[0] * rr))
        b = np.sqrt((v * v).sum(axis=1))
        moving = b > 0
        vhat = v / np.where(moving, b, 1.0)[:, None]
        pp = synth.lorentz_boost(v, np.stack([p[0], p[1], p[2], p[3]], axis=-1))
        a = np.where(moving, clamp((pp[:, 1:] * vhat).sum(axis=1) / pp[:, 0]), m)
        x = (v[:, 0] * p[1] + v[:, 1] * p[2] + v[:, 2] * p[3]) / p[0]
        bar_a = np.where(moving, 8 * U * (3 + np.abs(a) * b) / (1 - x), 0.0)
    return m, a, bar_a


def per_photon(frame, ph):
    """radfield_checker.per_photon's arrays (e_comv is e) and m, a, bar_a (NaN / 0 where there is no cell)"""
    q = rc.per_photon(frame, ph)
    f8 = lambda k: np.asarray(ph[k], dtype=np.float64)
    n = len(q["cell"])
    m, a, bar_a = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n)
    at = np.nonzero(q["cell"] >= 0)[0]
    if len(at):
        v = synth.hydro_vector_to_cartesian(frame, q["cell"][at], np.arctan2(f8("r1")[at], f8("r0")[at]))
        m[at], a[at], bar_a[at] = cosines(v, np.stack([f8(k)[at] for k in ("p0", "p1", "p2", "p3")]), np.stack([f8(k)[at] for k in ("r0", "r1", "r2")]))
    q.update(m=m, a=a, bar_a=bar_a, e=q["e_comv"])
    return q


def field(frame, ph, mode, e_edges, a_edges, r_edges=None, mu_edges=None):
    """-> dict: count, the seven sums and bound_<sum> per bin ((M, n_e, n_a) for CELLS, (n_r, n_mu, n_e, n_a) for SHELLS), count_sure (the count
    without the fragile photons), n_observable, n_unlocated, n_outside, n_fragile, and the per-photon arrays s, bin, fragile and q (per_photon's)"""
    q = per_photon(frame, ph)
    cell, e, a = q["cell"], q["e"], q["a"]
    e_edges, a_edges = np.asarray(e_edges, dtype=np.float64), np.asarray(a_edges, dtype=np.float64)
    n_e, n_a = len(e_edges) - 1, len(a_edges) - 1
    if mode == CELLS:
        pos_shape = (int(frame["num_elements"]),)
        s = cell.copy()
    else:
        n_r, n_mu = len(r_edges) - 1, len(mu_edges) - 1
        pos_shape = (n_r, n_mu)
        ir, imu = find_bin(r_edges, q["r"]), find_bin(mu_edges, q["mu"])
        s = np.where((cell >= 0) & (ir >= 0) & (imu >= 0), ir * n_mu + imu, -1)
    shape = pos_shape + (n_e, n_a)
    n_bins = int(np.prod(shape))
    ie, ia = find_bin(e_edges, e), find_bin(a_edges, a)
    bin_ = np.where((s >= 0) & (ie >= 0) & (ia >= 0), (s * n_e + ie) * n_a + ia, -1)
    de, da = 2 * q["bar_e"], 2 * q["bar_a"]
    with np.errstate(invalid="ignore"):
        on_edge = (find_bin(e_edges, e * (1 - de)) != find_bin(e_edges, e * (1 + de))) | (find_bin(a_edges, clamp(a - da)) != find_bin(a_edges, clamp(a + da)))
    fragile = q["near"] | ((cell >= 0) & on_edge)
    w = np.asarray(ph["weight"], dtype=np.float64)
    inb = np.nonzero(bin_ >= 0)[0]
    we, wl = w[inb] * e[inb], w[inb] * q["e_lab"][inb]
    ai, mi = a[inb], q["m"][inb]
    terms = {"w": w[inb], "we": we, "wea": we * ai, "weaa": (we * ai) * ai, "we_lab": wl, "wem": wl * mi, "wemm": (wl * mi) * mi}
    dei, dai = de[inb], da[inb]
    cond = {"we": dei * np.abs(we), "wea": (dei * np.abs(ai) + dai) * np.abs(we), "weaa": (dei * ai * ai + 2 * np.abs(ai) * dai + dai * dai) * np.abs(we)}
    out = {"count": np.bincount(bin_[inb], minlength=n_bins).astype(np.int64).reshape(shape)}
    sure = inb[~fragile[inb]]
    out["count_sure"] = np.bincount(bin_[sure], minlength=n_bins).astype(np.int64).reshape(shape)
    n_terms = out["count"].astype(np.float64)
    for k in SUMS:
        acc, mag = np.zeros(n_bins, dtype=np.longdouble), np.zeros(n_bins, dtype=np.longdouble)      # (the sums in extended precision: their own error is far below u)
        np.add.at(acc, bin_[inb], terms[k].astype(np.longdouble))
        np.add.at(mag, bin_[inb], np.abs(terms[k]).astype(np.longdouble))
        out[k] = acc.astype(np.float64).reshape(shape)
        bound = (n_terms + 2.0) * U * mag.astype(np.float64).reshape(shape)
        if k in cond:
            c = np.zeros(n_bins, dtype=np.longdouble)
            np.add.at(c, bin_[inb], cond[k].astype(np.longdouble))
            bound = bound + c.astype(np.float64).reshape(shape)
        out["bound_" + k] = bound
    obs = q["observable"]
    out.update(n_observable=int(obs.sum()), n_unlocated=int((obs & (cell < 0)).sum()), n_outside=int(((cell >= 0) & (bin_ < 0)).sum()),
               n_fragile=int(fragile.sum()), s=s, bin=bin_, fragile=fragile, q=q)
    return out


def add(results):
    """several fields of one binning added up: counts, sums, bounds and counters"""
    out = {}
    for k, v in results[0].items():
        if k in ("s", "bin", "fragile", "q"):
            continue
        out[k] = sum(r[k] for r in results[1:]) + v
    return out


def moments(res):
    """J, H, K per position bin in the fluid frame and in the lab (the sums over the e and a axes) and K / J, H / J; NaN where J == 0"""
    out = {}
    for tag, planes in (("", ("we", "wea", "weaa")), ("_lab", ("we_lab", "wem", "wemm"))):
        j, h, k = (np.asarray(res[p], dtype=np.float64).sum(axis=(-2, -1)) for p in planes)
        with np.errstate(invalid="ignore", divide="ignore"):
            out.update({"J" + tag: j, "H" + tag: h, "K" + tag: k, "K_over_J" + tag: np.where(j != 0, k / j, np.nan), "H_over_J" + tag: np.where(j != 0, h / j, np.nan)})
    return out


# ---------------------------------------------------------------------------------------------- the cases of the CPU and the GPU test
CYL = rc.CYL
SHELL_R, SHELL_MU = rc.SHELL_R, rc.SHELL_MU                    # radfield_checker's 8 x 4 shells
# six energy bins over the fluid-frame energies of the cases [erg] -- some photons lie below and above -- and four cosine bins with the forward pole
# closed; the energies of the cases are drawn continuously over four decades, so no photon sits on an edge by construction
E_EDGES = 10.0 ** np.linspace(-11.03, -4.97, 7)
A_EDGES = np.array([-1.0, -0.47, 0.03, 0.52, np.nextafter(1.0, 2.0)])


def at_rest(frame, cells):
    """the frame with the fluid of `cells` at rest (v = 0, gamma = 1)"""
    out = dict(frame)
    for k in ("v0", "v1", "v2"):
        if k in out:
            out[k] = out[k].copy()
            out[k][cells] = 0.0
    out["gamma"] = out["gamma"].copy()
    out["gamma"][cells] = 1.0
    out["dens"] = out["dens_lab"] / out["gamma"]
    return out


def _rest_case():
    c = rc._case(*CYL, 660, 1000)
    frame = at_rest(c["frame"], np.arange(0, c["frame"]["num_elements"], 3))
    return dict(frame=frame, whole=frame, ph=c["ph"])


def _build_cases():
    cases = {}
    for name in ("cells_n1", "cells_n63", "cells_n65", "cells_n1000", "gamma_100", "crowded_4", "crowded_1", "spread", "gap", "shells"):
        cases[name] = lambda name=name: rc.case(name)
    for dims, geom in PAIRS:
        cases["pair_%d_%d" % (dims, geom)] = lambda name="pair_%d_%d" % (dims, geom): rc.case(name)
    cases["cells_n257"] = lambda: rc._case(*CYL, 657, 257)
    cases["rest"] = _rest_case
    return cases


CASES = _build_cases()


@functools.lru_cache(maxsize=None)
def case(name):
    """the case's inputs, computed once per process: dict(frame, whole, ph)"""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def want(name, mode):
    """... and the checker's answer on the case's own frame, CELLS or SHELLS 8 x 4, with E_EDGES x A_EDGES (shared by the tests: do not change it)"""
    c = case(name)
    return field(c["frame"], c["ph"], mode, E_EDGES, A_EDGES, *((SHELL_R, SHELL_MU) if mode == SHELLS else ()))


# ---------------------------------------------------------------------------------------------- isotropic radiation in the fluid frame
def isotropic(n=4096, seed=700, e0=3.1e-8):
    """n equal-weight photons drawn isotropically, with the one energy e0 [erg], in the frame of the cell they sit in, and taken to the lab with the
    textbook boost by -v: the frame random_fluid(mesh(CYL), seed) (gamma up to 10), points in the middle of random cells
    -> dict(frame, ph, a_true: the cosines about the flow as drawn)"""
    frame = random_fluid(mesh(*CYL), seed)
    g = np.random.default_rng(seed + 1)
    cells = g.integers(0, frame["num_elements"], n)
    r = rc.points_in_cells(frame, cells, seed + 2)
    v = synth.hydro_vector_to_cartesian(frame, cells, np.arctan2(r[1], r[0]))
    d = g.standard_normal((n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    pc = np.concatenate([np.ones((n, 1)), d], axis=1) * (e0 / synth.C_LIGHT)
    lab = synth.lorentz_boost(-v, pc)
    ph = rc.photon_list(r, lab.T.copy(), seed + 3, exclusions=False)
    ph["weight"][:] = 1.0e49
    a_true = (d * v).sum(axis=1) / np.sqrt((v * v).sum(axis=1))
    return dict(frame=frame, ph=ph, a_true=a_true, cells=cells)
