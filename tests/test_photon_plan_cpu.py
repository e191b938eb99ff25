"""The host's rules for the photon storage (mcrat_amd/csrc/photon_plan.hpp) on the CPU: the column tables, the block's layout, a block bound to a
base address, a pool's windows, "the same block, elsewhere" (the snapshot and the captured frames), the copies that restore one list's window, the
derived columns and the flag byte of a list that comes in as columns, and the output block of get_output and the outbox.  Every kernel trusts the
PhotonDev these rules produce, so they are restated here and held against what the header computes.  Plain C++: a small driver is compiled with g++
and what it prints is compared -- integers and addresses exactly, doubles bit for bit (%a)."""
import itertools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_LIGHT = 2.99792458e10
STEP_BLOCK = 256
FLAG_RECALC, FLAG_MOVES, FLAG_VALID = 1, 2, 4
# PhotonDev's double columns in PhotonCol order (photon_cols.hpp); the first 19 cross the ABI under the names of mcrat_hip_photon_soa
DEV_COLS = ["r0", "r1", "r2", "p0", "p1", "p2", "p3", "c0", "c1", "c2", "c3", "s0", "s1", "s2", "s3", "num_scatt", "weight", "tau", "tts",
            "u0", "u1", "u2", "ntau", "tau_next"]
SOA_COLS = ["r0", "r1", "r2", "p0", "p1", "p2", "p3", "comv_p0", "comv_p1", "comv_p2", "comv_p3", "s0", "s1", "s2", "s3", "num_scatt", "weight",
            "total_optical_depth", "time_to_scatter"]
# the output columns in OutputCols order (staging.hip)
OUT_COLS = ["p0", "p1", "p2", "p3", "comv_p0", "comv_p1", "comv_p2", "comv_p3", "r0", "r1", "r2", "s0", "s1", "s2", "s3", "num_scatt", "weight"]

LAYOUT_N = [1, 511, 512, 513, 1000, 171798528, 171798529]        # 171 798 528: the last capacity with 25 x stride < 2^32
BASE = 0x7f0000001000                                            # a fake device address (nothing is dereferenced)
BIND_N = 1000
WINDOWS = [(stride, rank, n) for stride in (512, 1024) for rank in (0, 1, 3) for n in (0, 1, stride)]      # 4 ranks: 0, 1 and the last
CAP, CAP_FRAMES = 0x7e0000000000, 3
REPLAY = [(0, 1), (1, 300), (2, 512), (1, 0)]                    # (rank, n) in a block of 3 ranks x 512 slots
P0 = [1.0, 3.7, 0.0, 5e-324, 1e-310, -2.5, 1e300, 0.1]           # with p0 == 0 and two denormals
P1 = [0.5, -1.25, 2.0, 0.0, 3.0, 1e-3, 1e300, 0.1]
P2 = [0.25, 0.7, -1.0, 1.0, -2.0, 7.0, -1e300, 0.2]
P3 = [-0.75, 1e-20, 4.0, -1.0, 0.0, 0.3, 5.0, 0.3]
TAU = [2.0, 0.0, 1e-3, -0.0, 5e-324, 1e300, -4.0, 1.0 / 3.0]     # with tau == 0
FLAG_TYPES, FLAG_WEIGHTS, FLAG_RECALCS = "piNck", [0.0, -0.0, 1.0, -2.5, 5e-324, float("nan")], [0, 1, 2, -1]
OUTPUT = [(m, n_rec, want) for m in (0, 1, 32, 33) for n_rec in (0, 600) for want in (1,)] + [(0, 600, 0), (0, 0, 0)]
SCAN_INTS = 7

DRIVER = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "photon_plan.hpp"
using namespace mcrat;
typedef unsigned long long ull;
static ull addr(const void *p) { return (ull)(uintptr_t)p; }

static void dev(const char *key, const PhotonDev &p)
{
    // by member NAME, in the order of device_types.hpp: what the table must agree with
    const double *cols[24] = {p.r0, p.r1, p.r2, p.p0, p.p1, p.p2, p.p3, p.c0, p.c1, p.c2, p.c3, p.s0, p.s1, p.s2, p.s3, p.num_scatt, p.weight, p.tau, p.tts,
                              p.u0, p.u1, p.u2, p.ntau, p.tau_next};
    printf("%s:", key);
    for (int k = 0; k < 24; ++k) printf(" %llu", addr(cols[k]));
    printf(" %llu %llu %llu %d %d %u\n", addr(p.idx), addr(p.flags), addr(p.type), p.n, p.n_pad, p.col_stride);
}
static void layout(int n)
{
    PhotonLayout l;
    memset(&l, 0xff, sizeof l);
    const PhotonLayoutStatus st = photon_layout(n, &l);
    printf("layout_%d: %d", n, (int)st);
    if (st == PHOTON_LAYOUT_OK) {
        printf(" %d %u %zu", l.n_pad, l.col_stride, l.total);
        for (int k = 0; k < N_BLOCK_COLS; ++k) printf(" %zu", l.col[k]);
        printf(" %zu %zu %zu", l.idx, l.flags, l.type);
    }
    printf("\n");
    printf("layouttext_%d:%s\n", n, photon_layout_text(st));
}
static void output(size_t m, int n_records, int want)
{
    const OutputLayout l = output_layout(m, @SCAN_INTS@, n_records, want != 0);
    char key[64];
    snprintf(key, sizeof key, "output_%zu_%d_%d", m, n_records, want);
    printf("%s: %zu %zu", key, l.rec, l.rec_bytes);
    for (int k = 0; k < N_OUTPUT_COLS; ++k) printf(" %zu", l.col[k]);
    printf(" %zu %zu %zu %zu\n", l.type, l.scan, l.total, l.copy_bytes);
    mcrat_hip_output_columns c;
    memset(&c, 0, sizeof c);
    c.count = 12345;
    bind_output(l, (void *)(uintptr_t)@BASE@ull, &c);               // what mcrat_hip_outbox_wait hands out, by member name in OutputCols order
    const double *cols[17] = {c.p0, c.p1, c.p2, c.p3, c.comv_p0, c.comv_p1, c.comv_p2, c.comv_p3, c.r0, c.r1, c.r2, c.s0, c.s1, c.s2, c.s3, c.num_scatt, c.weight};
    printf("outbound_%zu_%d_%d:", m, n_records, want);
    for (int k = 0; k < 17; ++k) printf(" %llu", addr(cols[k]));
    printf(" %llu %d\n", addr(c.type), c.count);
}

int main()
{
    printf("counts: %d %d %d %d\n", N_PHOTON_COLS, N_ABI_COLS, N_BLOCK_COLS, N_OUTPUT_COLS);
    {   // the ABI tables: the address of the member each entry names, in a struct at address 0 .. as offsets
        mcrat_hip_photon_soa s;
        mcrat_hip_output_columns o;
        printf("soa_offsets:");
        for (int k = 0; k < N_ABI_COLS; ++k) printf(" %zu", (size_t)((char *)&(s.*SOA_COLS[k]) - (char *)&s));
        printf("\nsoa_named: %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(mcrat_hip_photon_soa, r0),
               offsetof(mcrat_hip_photon_soa, r1), offsetof(mcrat_hip_photon_soa, r2), offsetof(mcrat_hip_photon_soa, p0), offsetof(mcrat_hip_photon_soa, p1),
               offsetof(mcrat_hip_photon_soa, p2), offsetof(mcrat_hip_photon_soa, p3), offsetof(mcrat_hip_photon_soa, comv_p0),
               offsetof(mcrat_hip_photon_soa, comv_p1), offsetof(mcrat_hip_photon_soa, comv_p2), offsetof(mcrat_hip_photon_soa, comv_p3),
               offsetof(mcrat_hip_photon_soa, s0), offsetof(mcrat_hip_photon_soa, s1), offsetof(mcrat_hip_photon_soa, s2), offsetof(mcrat_hip_photon_soa, s3),
               offsetof(mcrat_hip_photon_soa, num_scatt), offsetof(mcrat_hip_photon_soa, weight), offsetof(mcrat_hip_photon_soa, total_optical_depth),
               offsetof(mcrat_hip_photon_soa, time_to_scatter));
        printf("out_offsets:");
        for (int k = 0; k < N_OUTPUT_COLS; ++k) printf(" %zu", (size_t)((char *)&(o.*OUTPUT_COLS[k]) - (char *)&o));
        printf("\nout_named: %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(mcrat_hip_output_columns, p0),
               offsetof(mcrat_hip_output_columns, p1), offsetof(mcrat_hip_output_columns, p2), offsetof(mcrat_hip_output_columns, p3),
               offsetof(mcrat_hip_output_columns, comv_p0), offsetof(mcrat_hip_output_columns, comv_p1), offsetof(mcrat_hip_output_columns, comv_p2),
               offsetof(mcrat_hip_output_columns, comv_p3), offsetof(mcrat_hip_output_columns, r0), offsetof(mcrat_hip_output_columns, r1),
               offsetof(mcrat_hip_output_columns, r2), offsetof(mcrat_hip_output_columns, s0), offsetof(mcrat_hip_output_columns, s1),
               offsetof(mcrat_hip_output_columns, s2), offsetof(mcrat_hip_output_columns, s3), offsetof(mcrat_hip_output_columns, num_scatt),
               offsetof(mcrat_hip_output_columns, weight));
    }
    const int layout_n[] = {@LAYOUT_N@};
    for (int n : layout_n) layout(n);
    {
        PhotonLayout l;
        photon_layout(@BIND_N@, &l);
        const PhotonDev p = bind_photons(l, (void *)(uintptr_t)@BASE@ull, @BIND_N@);
        dev("bind", p);
        printf("bind_table:");                                      // ... and through the table
        for (int k = 0; k < N_PHOTON_COLS; ++k) printf(" %llu", addr(p.*PHOTON_COLS[k]));
        printf("\n");
    }
    {
        const int windows[][3] = {@WINDOWS@};
        for (const auto &w : windows) {
            PhotonLayout l;
            photon_layout(4 * w[0], &l);
            const PhotonDev pool = bind_photons(l, (void *)(uintptr_t)@BASE@ull, 4 * w[0]);
            char key[64];
            snprintf(key, sizeof key, "pool_%d_%d_%d", w[0], w[1], w[2]);
            dev(key, pool);
            snprintf(key, sizeof key, "window_%d_%d_%d", w[0], w[1], w[2]);
            dev(key, photon_window(pool, w[1], w[0], w[2]));
        }
    }
    {   // the same block, elsewhere
        PhotonLayout l;
        photon_layout(3 * 512, &l);
        const PhotonDev live = bind_photons(l, (void *)(uintptr_t)@BASE@ull, 3 * 512);
        dev("live", live);
        printf("block_bytes: %zu\n", l.total);
        int round_trips = 0;
        for (int f = 0; f < @CAP_FRAMES@; ++f) {
            const long long d = image_delta((const void *)(uintptr_t)@CAP@ull, (const void *)(uintptr_t)@BASE@ull, f, l.total);
            const PhotonDev there = shift_photons(live, d), back = shift_photons(there, -d);
            char key[32];
            snprintf(key, sizeof key, "capture_%d", f);
            dev(key, there);
            round_trips += memcmp(&back, &live, sizeof live) == 0;
        }
        printf("round_trips: %d\n", round_trips);
    }
    {   // one list's window of the block back from an image of it, on host bytes
        PhotonLayout l;
        photon_layout(3 * 512, &l);
        printf("replay_layout: %zu", l.total);
        for (int k = 0; k < N_BLOCK_COLS; ++k) printf(" %zu", l.col[k]);
        printf(" %zu %zu %zu\n", l.idx, l.flags, l.type);
        const int lists[][2] = {@REPLAY@};
        for (const auto &q : lists) {
            std::vector<unsigned char> live(l.total), snap(l.total);
            for (size_t i = 0; i < l.total; ++i) { live[i] = (unsigned char)(i * 131 + 7); snap[i] = (unsigned char)~live[i]; }
            CopyExtent ext[N_WINDOW_EXTENTS];
            window_extents(l, (size_t)q[0] * 512, (size_t)q[1], ext);
            for (const CopyExtent &e : ext)
                for (size_t row = 0; row < e.rows; ++row) memcpy(&live[e.off + row * e.pitch], &snap[e.off + row * e.pitch], e.width);
            printf("replay_%d_%d:", q[0], q[1]);                     // the runs of bytes that changed: start, length
            for (size_t i = 0; i < l.total;) {
                if (live[i] == (unsigned char)(i * 131 + 7)) { ++i; continue; }
                size_t j = i;
                while (j < l.total && live[j] == (unsigned char)~(unsigned char)(j * 131 + 7)) ++j;
                printf(" %zu %zu", i, j - i);
                i = j;
            }
            printf("\n");
        }
    }
    {
        const double p0[] = {@P0@}, p1[] = {@P1@}, p2[] = {@P2@}, p3[] = {@P3@}, tau[] = {@TAU@};
        const int n = (int)(sizeof p0 / sizeof p0[0]);
        std::vector<double> out(4 * n, 12345.0);
        derived_columns(n, p0, p1, p2, p3, tau, out.data());
        printf("derived:");
        for (double v : out) printf(" %a", v);
        std::fill(out.begin(), out.end(), 12345.0);
        derived_columns(n, p0, p1, p2, p3, nullptr, out.data());
        printf("\nderived_no_tau:");
        for (double v : out) printf(" %a", v);
        printf("\n");
    }
    {
        const char types[] = "@FLAG_TYPES@";
        const double weights[] = {@FLAG_WEIGHTS@};
        const int recalcs[] = {@FLAG_RECALCS@};
        printf("flags:");
        for (const char *t = types; *t; ++t)
            for (double w : weights)
                for (int r : recalcs) printf(" %d", (int)make_flags(*t, w, r));
        printf("\n");
    }
@OUTPUT@
    return 0;
}
'''


def _cdouble(v):
    return "__builtin_nan(\"\")" if v != v else float(v).hex()      # (hex literals: the driver gets exactly these doubles)


def driver_source():
    """the driver with the cases filled in (also what a stand-alone sanitizer build compiles)"""
    subs = {"SCAN_INTS": str(SCAN_INTS), "BASE": "%d" % BASE, "CAP": "%d" % CAP, "CAP_FRAMES": str(CAP_FRAMES), "BIND_N": str(BIND_N),
            "LAYOUT_N": ", ".join(map(str, LAYOUT_N)), "WINDOWS": ", ".join("{%d, %d, %d}" % w for w in WINDOWS),
            "REPLAY": ", ".join("{%d, %d}" % q for q in REPLAY), "FLAG_TYPES": FLAG_TYPES, "FLAG_WEIGHTS": ", ".join(map(_cdouble, FLAG_WEIGHTS)),
            "FLAG_RECALCS": ", ".join(map(str, FLAG_RECALCS)), "OUTPUT": "\n".join("    output(%d, %d, %d);" % q for q in OUTPUT)}
    for name, vals in (("P0", P0), ("P1", P1), ("P2", P2), ("P3", P3), ("TAU", TAU)):
        subs[name] = ", ".join(map(_cdouble, vals))
    src = DRIVER
    for k, v in subs.items():
        src = src.replace("@%s@" % k, v)
    return src


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """what the driver printed: {key: [tokens]}"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("photon_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(driver_source())
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    res = {}
    for line in text.splitlines():
        key, _, vals = line.partition(":")
        res[key] = vals if key.startswith("layouttext_") else vals.split()
    return res


def ints(tokens):
    return [int(t) for t in tokens]


def align_up(x, a):
    return (x + a - 1) // a * a


def layout_rule(n):
    """the block as engine.hip's alloc_photons laid it out before the rule moved: capacity max(n, 1) rounded up to 2 * STEP_BLOCK, 25 double columns,
    idx, flags, type, each on a 256-byte boundary -> None where 25 x stride does not fit in 32 bits"""
    n_pad = align_up(max(n, 1), 2 * STEP_BLOCK)
    off, offs = 0, []
    for size in [8] * 25 + [4, 1, 1]:
        offs.append(off)
        off = align_up(off + size * n_pad, 256)
    stride = (offs[1] - offs[0]) // 8
    if stride * 25 > 0xffffffff:
        return None
    return {"n_pad": n_pad, "col_stride": stride, "total": off, "col": offs[:25], "idx": offs[25], "flags": offs[26], "type": offs[27]}


def dev_of(tokens):
    v = ints(tokens)
    return {"col": v[:24], "idx": v[24], "flags": v[25], "type": v[26], "n": v[27], "n_pad": v[28], "col_stride": v[29]}


def test_the_tables_name_the_members_in_order(out):
    assert ints(out["counts"]) == [len(DEV_COLS), len(SOA_COLS), len(DEV_COLS) + 1, len(OUT_COLS)] == [24, 19, 25, 17]
    assert out["soa_offsets"] == out["soa_named"] and len(set(out["soa_offsets"])) == 19
    assert out["out_offsets"] == out["out_named"] and len(set(out["out_offsets"])) == 17
    assert out["bind_table"] == out["bind"][:24]                   # PHOTON_COLS[k] is the k-th member of PhotonDev, by name


@pytest.mark.parametrize("n", LAYOUT_N)
def test_photon_layout(out, n):
    got, want = ints(out["layout_%d" % n]), layout_rule(n)
    if n == 171798529:
        assert want is None
    if want is None:
        assert got == [1] and out["layouttext_%d" % n] == "photon list: more than 2^32 / 25 slots"
        return
    assert got[0] == 0 and out["layouttext_%d" % n] == ""
    n_pad, col_stride, total, col, (idx, flags, typ) = got[1], got[2], got[3], got[4:29], got[29:32]
    assert (n_pad, col_stride, total, col, idx, flags, typ) == (want["n_pad"], want["col_stride"], want["total"], want["col"], want["idx"], want["flags"], want["type"])
    assert n_pad >= max(n, 1) and n_pad % (2 * STEP_BLOCK) == 0 and n_pad - max(n, 1) < 2 * STEP_BLOCK
    assert col_stride == n_pad and col_stride * 25 <= 0xffffffff
    assert all(o % 256 == 0 for o in col + [idx, flags, typ, total])
    assert all(col[k] == col[0] + k * col_stride * 8 for k in range(25))         # equally spaced: what ListCols relies on
    regions = [(o, 8 * n_pad) for o in col] + [(idx, 4 * n_pad), (flags, n_pad), (typ, n_pad)]
    for (a, la), (b, _) in zip(regions, regions[1:] + [(total, 0)]):
        assert a + la <= b                                                       # in this order, none into the next, all inside the block
    if n == 171798528:
        assert n_pad == n and col_stride * 25 == 4294963200


def test_bind_photons(out):
    p, l = dev_of(out["bind"]), layout_rule(BIND_N)
    assert p["col"] == [BASE + k * l["col_stride"] * 8 for k in range(24)]
    assert (p["idx"], p["flags"], p["type"]) == (BASE + l["idx"], BASE + l["flags"], BASE + l["type"])
    assert (p["n"], p["n_pad"], p["col_stride"]) == (BIND_N, l["n_pad"], l["col_stride"]) == (1000, 1024, 1024)


@pytest.mark.parametrize("stride,rank,n", WINDOWS)
def test_photon_window(out, stride, rank, n):
    key = "%d_%d_%d" % (stride, rank, n)
    pool, w = dev_of(out["pool_" + key]), dev_of(out["window_" + key])
    first = rank * stride
    assert w["col"] == [a + 8 * first for a in pool["col"]]                      # every pointer by `first` elements of its own type
    assert (w["idx"], w["flags"], w["type"]) == (pool["idx"] + 4 * first, pool["flags"] + first, pool["type"] + first)
    assert (w["n"], w["n_pad"], w["col_stride"]) == (n, stride, pool["col_stride"]) and pool["col_stride"] == 4 * stride


def test_the_same_block_elsewhere(out):
    live, block = dev_of(out["live"]), int(out["block_bytes"][0])
    assert block == layout_rule(3 * 512)["total"]
    for f in range(CAP_FRAMES):
        there = dev_of(out["capture_%d" % f])
        for k in ("idx", "flags", "type"):
            assert there[k] == CAP + f * block + (live[k] - BASE)
        assert there["col"] == [CAP + f * block + (a - BASE) for a in live["col"]]
        assert (there["n"], there["n_pad"], there["col_stride"]) == (live["n"], live["n_pad"], live["col_stride"])
    assert ints(out["round_trips"]) == [CAP_FRAMES]                              # a shift and its inverse give back the original


@pytest.mark.parametrize("rank,n", REPLAY)
def test_window_copies_touch_exactly_the_lists_slots(out, rank, n):
    v = ints(out["replay_layout"])
    total, col, (idx, flags, typ) = v[0], v[1:26], v[26:29]
    l = layout_rule(3 * 512)
    assert (total, col, idx, flags, typ) == (l["total"], l["col"], l["idx"], l["flags"], l["type"])
    first = rank * 512
    want = [(col[k] + 8 * first, 8 * n) for k in range(24)] + [(idx + 4 * first, 4 * n), (flags + first, n), (typ + first, n)] if n else []
    got = ints(out["replay_%d_%d" % (rank, n)])
    assert list(zip(got[0::2], got[1::2])) == want                               # the 24 columns (not the scratch column) and idx, flags, type


def _bits(x):
    return struct.pack("<d", x)


def _same_doubles(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert _bits(g) == _bits(w) or (g != g and w != w), (got, want)


def derived_rule(tau):
    """upload_columns as it was: 1.0 / p0, then p_k * d * C_LIGHT (u = 0 where p0 == 0); -1.0 / tau, a missing tau as 0"""
    f8 = np.float64
    u = [[], [], []]
    with np.errstate(all="ignore"):
        for i, p0 in enumerate(P0):
            d = f8(1.0) / f8(p0) if p0 != 0 else None
            for k, col in enumerate((P1, P2, P3)):
                u[k].append(float(f8(col[i]) * d * f8(C_LIGHT)) if d is not None else 0.0)
        ntau = [float(f8(-1.0) / f8(t)) for t in (tau if tau is not None else [0.0] * len(P0))]
    return u[0] + u[1] + u[2] + ntau


def test_derived_columns(out):
    want = derived_rule(TAU)
    _same_doubles([float.fromhex(t) if "n" not in t else float(t) for t in out["derived"]], want)
    n = len(P0)
    assert want[2] == 0.0 and want[n + 2] == 0.0 and want[2 * n + 2] == 0.0                      # p0 == 0
    assert want[3 * n + 1] == float("-inf") and want[3 * n + 3] == float("inf")                  # tau == 0, tau == -0
    assert want[3] != want[3] and want[n + 3] == float("inf")                                    # a denormal p0: 1 / p0 overflows; 0 * inf
    want = derived_rule(None)
    _same_doubles([float.fromhex(t) if "n" not in t else float(t) for t in out["derived_no_tau"]], want)
    assert want[3 * n:] == [float("-inf")] * n


def test_make_flags(out):
    want = []
    for t, w, r in itertools.product(FLAG_TYPES, FLAG_WEIGHTS, FLAG_RECALCS):
        want.append(FLAG_VALID | (FLAG_MOVES if (t != "p" and w != 0) else 0) | (FLAG_RECALC if r == 1 else 0))
    assert ints(out["flags"]) == want
    assert set(want) == {4, 5, 6, 7}


@pytest.mark.parametrize("m,n_rec,want_output", OUTPUT)
def test_output_layout(out, m, n_rec, want_output):
    v = ints(out["output_%d_%d_%d" % (m, n_rec, want_output)])
    rec, rec_bytes, col, typ, scan, total, copy_bytes = v[0], v[1], v[2:19], v[19], v[20], v[21], v[22]
    # as mcrat_hip_outbox_post laid it out before the rule moved (mcrat_hip_get_output: the same without records, and m > 0)
    room = m if m else 1
    stride = align_up(8 * room, 256)
    want_rec = align_up(176 * n_rec, 256)
    cols_bytes = 17 * stride + align_up(room, 256) if want_output else 0
    scan_bytes = align_up(4 * SCAN_INTS, 256) if want_output else 0
    assert (rec, rec_bytes) == (0, want_rec)
    assert total == want_rec + cols_bytes + scan_bytes
    assert copy_bytes == want_rec + (cols_bytes if m > 0 else 0)
    b = ints(out["outbound_%d_%d_%d" % (m, n_rec, want_output)])
    assert b[18] == 12345                                                        # (count is the caller's)
    if not want_output:
        return
    assert col == [want_rec + k * stride for k in range(17)] and typ == want_rec + 17 * stride and scan == want_rec + cols_bytes
    regions = [(rec, 176 * n_rec)] + [(o, 8 * m) for o in col] + [(typ, m), (scan, 4 * SCAN_INTS)]
    assert all(o % 256 == 0 for o, _ in regions) and total % 256 == 0
    for (a, la), (nxt, _) in zip(regions, regions[1:] + [(total, 0)]):
        assert a + la <= nxt
    assert b[:17] == [BASE + o for o in col] and b[17] == BASE + typ             # wait()'s view of the columns is where post() wrote them
