"""The launch form of rank_loop_kernel (mcrat_amd/csrc/rank_form_plan.hpp) on the CPU: which builds of the kernel exist, which of them a request
resolves to and with how much LDS, the grid of a queue launch, and the engine's choice of threads per list.  The functions are plain C++: a small
driver is compiled with g++ and what it prints is compared with the rules of rank_form_plan.hpp's comments, restated here.  The launch forms that the
GPU tests drive by hand (tests/test_gpu_instantiations.py, tests/test_gpu_queue_instantiations.py) are held to the same rule."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARTESIAN, SPHERICAL, CYLINDRICAL, POLAR = 0, 1, 2, 3
GLOBAL = 1 << 30                                  # RANK_COLUMNS_GLOBAL
THREADS = (0, 64, 100, 128, 256, 512)
LONGEST = (64, 137, 1024, 1025, 1088, 1089, 4096, 4097, GLOBAL)
CUS = 256

DRIVER = r'''
#include <cstdio>
#include "rank_form_plan.hpp"
using namespace mcrat;

static void resolve_cases()
{
    const int threads[] = {0, 64, 100, 128, 256, 512};
    const int longest[] = {64, 137, 1024, 1025, 1088, 1089, 4096, 4097, RANK_COLUMNS_GLOBAL};
    for (int geom = 0; geom < 4; ++geom) for (int table = 0; table < 2; ++table) for (int stokes = 0; stokes < 2; ++stokes)
    for (int t : threads) for (int fuse = 0; fuse < 2; ++fuse) for (int hook = 0; hook < 2; ++hook) for (int queued = 0; queued < 2; ++queued)
    for (int nolds = 0; nolds < 2; ++nolds) for (int l : longest) {
        const RankFormPlan p = rank_form_resolve(RankFormRequest{t, fuse != 0, hook != 0, queued != 0, l, stokes != 0, geom, table != 0, nolds != 0});
        const RankForm &f = p.form;
        printf("resolve %d %d %d %d %d %d %d %d %d : %d %d %d %d %d %d %d %zu %d %d\n", geom, table, stokes, t, fuse, hook, queued, nolds, l,
               (int)f.stokes, (int)f.resident, f.threads, (int)f.fuse, (int)f.hook, (int)f.queue, p.lds_slots, p.dyn_bytes, (int)p.no_queue_build,
               (int)rank_build_exists(geom, table != 0, f.resident, f.threads, f.fuse, f.hook, f.queue, false));
    }
}

static void exists_cases()
{
    const int threads[] = {32, 64, 128, 256, 512, 1024};
    for (int geom = 0; geom < 4; ++geom) for (int table = 0; table < 2; ++table)
    for (int res = 0; res < 2; ++res) for (int t : threads) for (int fuse = 0; fuse < 2; ++fuse) for (int hook = 0; hook < 2; ++hook)
    for (int queue = 0; queue < 2; ++queue) for (int tape = 0; tape < 2; ++tape)
        if (rank_build_exists(geom, table != 0, res != 0, t, fuse != 0, hook != 0, queue != 0, tape != 0))
            printf("exists %d %d %d %d %d %d %d %d\n", geom, table, res, t, fuse, hook, queue, tape);
}

static RankEnv env_of(int block, int fuse)       // (-1: unset)
{
    RankEnv e;
    if (block >= 0) { e.block_set = true; e.block = block; }
    if (fuse >= 0) { e.fuse_set = true; e.fuse = fuse; }
    return e;
}

static void block_cases()
{
    const int cus = 256;
    const int ranks[] = {1, 200, 320, 321, 512, 513, 3071, 3072};
    const double passes[] = {0.0, 47.9, 48.0, 500.0};
    const int longest[] = {64, 1024, 1025, 1089, 5000};
    const int geoms[] = {GEOM_SPHERICAL, GEOM_CYLINDRICAL};
    const int blocks[] = {-1, 0, 7, 64, 128, 256, 512};
    for (int n : ranks) for (double pp : passes) for (int l : longest) for (int g : geoms) for (int b : blocks) for (int fuse = -1; fuse < 2; ++fuse) {
        const RankBlock r = rank_block_rule(n, cus, l, pp, g, env_of(b, fuse));
        printf("block %d %.17g %d %d %d %d : %d %d\n", n, pp, l, g, b, fuse, r.threads, (int)r.fuse);
    }
    const int cs_ranks[] = {1, 512, 513, 2048, 2049, 10000};
    for (int n : cs_ranks) for (int hook_kernel = 0; hook_kernel < 2; ++hook_kernel) for (int b : blocks) for (int fuse = -1; fuse < 2; ++fuse) {
        const RankBlock r = cs_rank_block_rule(n, cus, hook_kernel != 0, env_of(b, fuse));
        printf("csblock %d %d %d %d : %d %d\n", n, hook_kernel, b, fuse, r.threads, (int)r.fuse);
    }
}

static void grid_cases()
{
    const int c[][3] = {{100, 0, 256}, {100, 2, 0}, {100, 0, 0}, {100, 2, 256}, {511, 2, 256}, {512, 2, 256}, {513, 2, 256}, {100000, 2, 256}, {1, 8, 256}};
    for (const auto &k : c) printf("grid %d %d %d : %d\n", k[0], k[1], k[2], rank_queue_grid(k[0], k[1], k[2]));
}

int main()
{
    static_assert(rank_build_exists(GEOM_CARTESIAN, false, true, 256, true, false, true, false), "usable in a constant expression");
    printf("consts %d %d %d %d %d %d %d\n", GEOM_CARTESIAN, GEOM_SPHERICAL, GEOM_CYLINDRICAL, GEOM_POLAR, RANK_COLUMNS_GLOBAL, RANK_SMALL,
           rank_lds_bytes_per_slot(256) * 1000 + rank_lds_bytes_per_slot(128));
    resolve_cases();
    exists_cases();
    block_cases();
    grid_cases();
    return 0;
}
'''


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """what the driver printed: {tag: [(inputs, outputs)]}, numbers as the driver wrote them"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the planning functions' driver")
    d = tmp_path_factory.mktemp("rank_form_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    res = {}
    num = lambda v: float(v) if any(ch in v for ch in ".e") else int(v)
    for line in text.splitlines():
        tag, _, rest = line.partition(" ")
        ins, _, outs = rest.partition(" : ")
        res.setdefault(tag, []).append((tuple(num(v) for v in ins.split()), tuple(num(v) for v in outs.split())))
    assert res["consts"] == [((CARTESIAN, SPHERICAL, CYLINDRICAL, POLAR, GLOBAL, 128, 61032), ())]
    return res


# ---------------------------------------------------------------- the rules, restated

def build_exists(geom, table, resident, threads, fuse, hook, queue, tape):
    """tape: one form; hook: 64 / 128 / 256 threads, nothing else; fused: DIRECT, not spherical, 256 or 512 threads; queue: 256 threads in LDS"""
    if tape:
        return threads == 256 and not (resident or fuse or hook or queue)
    if hook:
        return threads in (64, 128, 256) and not (resident or fuse or queue)
    if fuse and (table or geom == SPHERICAL or threads not in (256, 512)):
        return False
    if queue:
        return threads == 256 and resident
    return threads in (128, 256, 512)


def resolve(geom, table, stokes, threads, fuse, hook, queued, nolds, longest):
    if not (threads == 128 or (threads == 64 and hook) or (threads == 512 and not hook)):
        threads = 256
    slots = 0
    if not hook and not nolds and longest <= {128: 1024, 256: 1088, 512: 4096}[threads]:
        slots = -(-longest // 16) * 16
    resident = slots > 0
    fuse = bool(fuse) and build_exists(geom, table, resident, threads, True, hook, queued, False)
    no_queue = bool(queued) and not build_exists(geom, table, resident, threads, fuse, hook, True, False)
    return (stokes, int(resident), threads, int(fuse), hook, queued, slots, slots * (61 if threads == 256 else 32), int(no_queue))


def block_rule(n, cus, passes, longest, geom, block, fuse):
    if block >= 0:
        threads = block if block in (128, 512) else 256
        fused = passes < 48.0
    else:
        small = (n > 2 * cus and passes >= 48.0) or n >= 12 * cus
        threads = 128 if small and longest <= 1024 else 256
        if longest > 1088 and n <= cus + cus // 4:
            threads = 512
        fused = passes < 48.0 and geom != SPHERICAL
    if fuse >= 0:
        fused = fuse != 0
    return threads, int(fused)


def cs_block_rule(n, cus, hook_kernel, block):
    threads = 128 if n > 2 * cus else 256
    if n > 8 * cus and not hook_kernel:
        threads = 64
    if block >= 0:
        threads = block if block in (64, 128) else 256
    return threads, 0


# ---------------------------------------------------------------- resolve

def test_every_request_resolves_as_the_rule_says(out):
    rows = out["resolve"]
    want_ins = list(itertools.product(range(4), (0, 1), (0, 1), THREADS, (0, 1), (0, 1), (0, 1), (0, 1), LONGEST))
    assert [r[0] for r in rows] == want_ins                                          # every combination, once
    for ins, got in rows:
        assert got[:9] == resolve(*ins), ins
    by = {r[0]: r[1] for r in rows}
    # the figures of the rule's comments: 137 slots round up to 144; 61 B per slot at 256 threads, 32 B otherwise; the limits 1024 / 1088 / 4096
    assert by[(CYLINDRICAL, 0, 0, 256, 1, 0, 0, 0, 137)][:9] == (0, 1, 256, 1, 0, 0, 144, 144 * 61, 0)
    assert by[(CYLINDRICAL, 0, 1, 128, 1, 0, 0, 0, 137)][:9] == (1, 1, 128, 0, 0, 0, 144, 144 * 32, 0)      # (128 threads: no fused build)
    assert by[(CYLINDRICAL, 0, 0, 512, 1, 0, 0, 0, 137)][:9] == (0, 1, 512, 1, 0, 0, 144, 144 * 32, 0)
    for threads, limit in ((128, 1024), (256, 1088), (512, 4096), (0, 1088), (100, 1088), (64, 1088)):
        for longest in LONGEST:
            slots = by[(CARTESIAN, 0, 0, threads, 0, 0, 0, 0, longest)][6]
            assert slots == ((longest + 15) // 16 * 16 if longest <= limit else 0), (threads, longest)
    for ins, got in rows:
        geom, table, stokes, threads, fuse, hook, queued, nolds, longest = ins
        if hook or nolds or longest == GLOBAL:
            assert got[1] == 0 and got[6] == 0 and got[7] == 0, ins                  # never resident: the hook, the switch (set to anything), the marker
        if fuse and (table or geom == SPHERICAL or hook or got[2] == 128):
            assert got[3] == 0, ins                                                  # the fused request that runs unfused


def test_every_resolved_form_is_a_build_or_a_queue_refusal(out):
    for ins, got in out["resolve"]:
        queued = ins[6]
        stokes, resident, threads, fuse, hook, queue, slots, dyn, no_queue, exists = got
        assert queue == queued
        if not queued:
            assert exists == 1 and no_queue == 0, ins
        else:
            assert no_queue == 1 - exists, ins
            assert bool(no_queue) == (threads != 256 or not resident), ins           # queue builds: 256-thread lists with their columns in LDS


# ---------------------------------------------------------------- the builds that exist are the builds that can be selected

def _existing(out):
    """{(geom, table): {(resident, threads, fuse, hook, queue, tape)}}, and the driver's list against the restated rule"""
    got = {}
    for ins, _ in out["exists"]:
        got.setdefault(ins[:2], set()).add(ins[2:])
    for geom, table in itertools.product(range(4), (0, 1)):
        want = {f for f in itertools.product((0, 1), (32, 64, 128, 256, 512, 1024), (0, 1), (0, 1), (0, 1), (0, 1)) if build_exists(geom, table, *f)}
        assert got[(geom, table)] == want, (geom, table)
    return got


def test_no_dead_builds(out):
    from tests.test_gpu_instantiations import PAIRS
    existing = _existing(out)
    total = 0
    for geom, table, stokes in itertools.product(range(4), (0, 1), (0, 1)):
        selected = {(False, 256, False, False, False, True)}                         # the tape build (launch_rank_loop_tape)
        for ins, got in out["resolve"]:
            if ins[:3] == (geom, table, stokes) and not got[8]:
                assert got[0] == stokes
                selected.add(tuple(got[1:6]) + (0,))
        assert selected == existing[(geom, table)], (geom, table, stokes)
        assert len(selected) == (16 if not table and geom != SPHERICAL else 11)
        total += len(selected) * sum(1 for _, g in PAIRS if g == geom)
    print("rank_loop_kernel instantiations the rule implies: %d" % total)
    assert total == 456                       # 16 per (pair, stokes) for DIRECT non-spherical, 11 for spherical and for TABLE, over the 9 pairs


# ---------------------------------------------------------------- threads per list

def test_rank_block_rule(out):
    by = {}
    for ins, got in out["block"]:
        n, passes, longest, geom, block, fuse = ins
        assert got == block_rule(n, CUS, passes, longest, geom, block, fuse), ins
        by[ins] = got
    cyl, sph = CYLINDRICAL, SPHERICAL
    # more than 2 x cus short lists and a dense last frame: 128 threads; from 12 x cus lists on whatever the frame looked like
    assert by[(512, 48.0, 64, cyl, -1, -1)] == (256, 0) and by[(513, 48.0, 64, cyl, -1, -1)] == (128, 0)
    assert by[(513, 47.9, 64, cyl, -1, -1)] == (256, 1) and by[(3071, 47.9, 64, cyl, -1, -1)] == (256, 1) and by[(3072, 47.9, 64, cyl, -1, -1)] == (128, 1)
    assert by[(3072, 48.0, 1024, cyl, -1, -1)] == (128, 0) and by[(3072, 48.0, 1025, cyl, -1, -1)] == (256, 0)
    # lists too long for LDS with 256 threads, about as many as CUs: 512 threads
    assert by[(320, 48.0, 1089, cyl, -1, -1)] == (512, 0) and by[(321, 48.0, 1089, cyl, -1, -1)] == (256, 0)
    # the fused pass: thin frames, not in spherical geometry -- unless MCRAT_HIP_RANK_BLOCK is set (resolve drops it there) or MCRAT_HIP_RANK_FUSE says
    assert by[(200, 47.9, 64, sph, -1, -1)] == (256, 0) and by[(200, 47.9, 64, cyl, -1, -1)] == (256, 1)
    assert by[(200, 47.9, 64, sph, 256, -1)] == (256, 1) and by[(200, 48.0, 64, sph, 256, -1)] == (256, 0)
    assert by[(200, 47.9, 64, cyl, -1, 0)] == (256, 0) and by[(200, 500.0, 64, sph, -1, 1)] == (256, 1) and by[(200, 500.0, 64, sph, 128, 1)] == (128, 1)
    # the override: 128 and 512 as they are, anything else (0 and 64 too) 256, whatever the lists look like
    for n, longest in ((1, 64), (3072, 64), (200, 5000)):
        assert [by[(n, 48.0, longest, cyl, b, -1)][0] for b in (128, 512, 7, 0, 64, 256)] == [128, 512, 256, 256, 256, 256]


def test_cs_rank_block_rule(out):
    by = {}
    for ins, got in out["csblock"]:
        n, hook_kernel, block, fuse = ins
        assert got == cs_block_rule(n, CUS, hook_kernel, block), ins                 # (MCRAT_HIP_RANK_FUSE is not looked at: these lists never fuse)
        by[ins] = got
    assert [by[(n, 0, -1, -1)][0] for n in (512, 513, 2048, 2049)] == [256, 128, 128, 64]
    assert [by[(n, 1, -1, -1)][0] for n in (512, 513, 2048, 2049)] == [256, 128, 128, 128]      # the hook as a kernel is written for 128 threads and more
    assert [by[(2049, 0, b, -1)][0] for b in (64, 128, 7, 512, 0)] == [64, 128, 256, 256, 256]
    assert by[(1, 1, 64, 1)] == (64, 0)


def test_queue_grid(out):
    got = {ins: g[0] for ins, g in out["grid"]}
    for (n_open, per_cu, cus), grid in got.items():
        assert grid == (min(n_open, per_cu * cus) if per_cu > 0 and cus > 0 else n_open)
    assert got[(100, 0, 256)] == got[(100, 2, 0)] == got[(100, 0, 0)] == got[(100, 2, 256)] == 100      # unknown per_cu or cus; fewer items than the device holds
    assert got[(512, 2, 256)] == 512 and got[(513, 2, 256)] == 512 and got[(100000, 2, 256)] == 512


# ---------------------------------------------------------------- the launch forms the GPU tests drive are the rule's

def test_the_gpu_tests_drive_the_forms_the_rule_allows(out):
    from mcrat_amd import synth
    from tests import test_gpu_instantiations as inst, test_gpu_queue_instantiations as queue
    assert (synth.CARTESIAN, synth.SPHERICAL, synth.CYLINDRICAL, synth.POLAR) == (CARTESIAN, SPHERICAL, CYLINDRICAL, POLAR)
    existing = _existing(out)
    for geom, table in itertools.product(range(4), (0, 1)):
        keyed = {(threads, fuse, resident) for resident, threads, fuse, hook, q, tape in existing[(geom, table)] if not (hook or q or tape)}
        forms = inst._forms(table, geom)
        assert len(forms) == len(set(forms)) and set(forms) == keyed, (geom, table)
        queued = {fuse for resident, threads, fuse, hook, q, tape in existing[(geom, table)] if q}
        assert all((1, 256, fuse, 0, 1, 0) in existing[(geom, table)] for fuse in queued)
        assert sorted(queue._queue_forms(table, geom)) == sorted(queued), (geom, table)
    # ... and each of them is what the switches those tests set resolve to (MCRAT_HIP_RANK_BLOCK, MCRAT_HIP_RANK_FUSE, MCRAT_HIP_NO_LDS_LISTS)
    by = {r[0]: r[1] for r in out["resolve"]}
    longest = 137
    assert longest in inst.LENS and max(inst.LENS) <= 1024                           # (the tests' lists are below every LDS limit, as 137 is)
    for (geom, table), stokes in itertools.product(existing, (0, 1)):
        for threads, fuse, lds in inst._forms(table, geom):
            assert by[(geom, table, stokes, threads, fuse, 0, 0, 1 - lds, longest)][1:4] == (lds, threads, fuse)
        for fuse in queue._queue_forms(table, geom):
            assert by[(geom, table, stokes, 256, fuse, 0, 1, 0, longest)][1:4] + by[(geom, table, stokes, 256, fuse, 0, 1, 0, longest)][8:9] == (1, 256, fuse, 0)
