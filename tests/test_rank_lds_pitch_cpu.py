"""The dynamic LDS a resident launch of rank_loop_kernel asks for (mcrat_amd/csrc/rank_form_plan.hpp: rank_lds_limit, RankFormPlan::lds_bytes) on the
CPU.  The kernel reaches the LDS copy's columns a compile-time pitch apart -- the launch form's slot limit -- so the launch's size is the limit's
whatever the lists' length: the last column ends at pitch x bytes per slot.  dyn_bytes stays what the lists' own slots hold.  Plain C++: a small
driver is compiled with g++ and what it prints is compared with the rule restated here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOBAL = 1 << 30
THREADS = (64, 128, 256, 512, 100)
LONGEST = (1, 16, 137, 1000, 1024, 1025, 1072, 1073, 1088, 1089, 4096, 4097, GLOBAL)
LIMIT = {128: 1024, 256: 1088, 512: 4096}
BYTES = {128: 32, 256: 61, 512: 32}
STATIC = {128: 7 * 1024, 256: 13 * 1024, 512: 27 * 1024}       # static LDS of the builds, rounded up (profiles/column_addressing_before_after.txt)
PER_CU = {128: 4, 256: 2, 512: 1}

DRIVER = r'''
#include <cstdio>
#include "rank_form_plan.hpp"
using namespace mcrat;
int main()
{
    static_assert(rank_lds_limit(256) == 1088, "usable in a constant expression");
    const int threads[] = {@THREADS@}, longest[] = {@LONGEST@};
    for (int t : threads) printf("limit %d : %d %d\n", t, rank_lds_limit(t), rank_lds_bytes_per_slot(t));
    for (int t : threads) for (int hook = 0; hook < 2; ++hook) for (int queued = 0; queued < 2; ++queued) for (int nolds = 0; nolds < 2; ++nolds) for (int l : longest) {
        const RankFormPlan p = rank_form_resolve(RankFormRequest{t, true, hook != 0, queued != 0, l, false, GEOM_CYLINDRICAL, false, nolds != 0});
        printf("plan %d %d %d %d %d : %d %d %d %zu %zu\n", t, hook, queued, nolds, l, p.form.threads, (int)p.form.resident, p.lds_slots, p.dyn_bytes, p.lds_bytes);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rule's driver")
    d = tmp_path_factory.mktemp("rank_lds_pitch")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER.replace("@THREADS@", ", ".join(map(str, THREADS))).replace("@LONGEST@", ", ".join(map(str, LONGEST))))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    res = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        tag, _, rest = line.partition(" ")
        ins, _, outs = rest.partition(" : ")
        res.setdefault(tag, {})[tuple(int(v) for v in ins.split())] = tuple(int(v) for v in outs.split())
    return res


def test_the_pitch_is_the_slot_limit_and_the_lists_per_cu_still_fit(out):
    for block in LIMIT:
        assert out["limit"][(block,)] == (LIMIT[block], BYTES[block])
    for block in LIMIT:
        assert PER_CU[block] * (STATIC[block] + LIMIT[block] * BYTES[block]) <= 160 * 1024, block
    # seven double columns of 1088 slots, then the cell index, then the flags: the last column starts inside the 64 KB a DS immediate reaches
    assert 7 * 8 * 1088 + 4 * 1088 < 1 << 16


def test_a_resident_launch_asks_for_the_limits_bytes(out):
    assert len(out["plan"]) == len(THREADS) * 8 * len(LONGEST)
    for (t, hook, queued, nolds, longest), (threads, resident, slots, dyn, lds) in out["plan"].items():
        block = threads
        want_resident = not hook and not nolds and longest <= LIMIT.get(block, 1088)
        assert resident == int(want_resident), (t, hook, queued, nolds, longest)
        if resident:
            assert slots == -(-longest // 16) * 16 <= LIMIT[block]
            assert dyn == slots * BYTES[block] <= lds == LIMIT[block] * BYTES[block]
        else:
            assert (slots, dyn, lds) == (0, 0, 0)
    by = out["plan"]
    assert by[(256, 0, 1, 0, 1000)][2:] == (1008, 1008 * 61, 66368)                  # the benchmark's lists: below the pitch
    assert by[(256, 0, 1, 0, 1088)][2:] == (1088, 66368, 66368)                      # at the pitch
    assert by[(128, 0, 0, 0, 1024)][2:] == (1024, 32768, 32768) and by[(512, 0, 0, 0, 137)][2:] == (144, 144 * 32, 131072)


def test_the_launch_is_sized_by_the_builds_thread_count(tmp_path):
    """-DRANK_SMALL=64 (the A/B of one-wave lists): a request for 128 threads runs the 64-thread build, whose kernel takes its pitch from ITS thread
    count -- 1088 slots, not the request's 1024 -- so the launch must ask for 1088 x 32 B: with 1024 x 32 the last column of a 1024-photon list would
    run 1536 B past the launch's LDS"""
    src, exe = tmp_path / "small.cpp", tmp_path / "small"
    src.write_text(r'''
#include <cstdio>
#include "rank_form_plan.hpp"
using namespace mcrat;
int main()
{
    const RankFormPlan p = rank_form_resolve(RankFormRequest{128, false, false, false, 1024, false, GEOM_CYLINDRICAL, false, false});
    printf("%d %d %zu %zu %d %d\n", p.form.threads, p.lds_slots, p.dyn_bytes, p.lds_bytes, rank_lds_limit(p.form.threads), rank_lds_bytes_per_slot(p.form.threads));
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DRANK_SMALL=64", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    threads, slots, dyn, lds, pitch, per_slot = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (threads, slots, dyn) == (64, 1024, 1024 * 32)
    assert lds == pitch * per_slot == 1088 * 32
    assert 3 * pitch * 8 + slots * 8 <= lds                                          # the fourth (last) double column of the longest list ends inside
