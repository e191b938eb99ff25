"""How the loop kernel addresses a slot of a global photon column (mcrat_amd/csrc/photon_plan.hpp, photon_addressing) on the CPU: a slot's 32-bit byte
offset i * 8 beside the column's scalar base where every offset of the block fits (n_pad * 8 < 2^32), the 32-bit index k * col_stride + i -- the
accessor before byte offsets -- where not.  The rule is plain C++: a small driver is compiled with g++ and what it prints is compared with the rule
restated here, one slot on either side of n_pad * 8 = 2^32, and with photon_layout's own bound, which is the tighter one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX, BYTE_OFFSET = 0, 1
EDGE = 1 << 29                                    # n_pad * 8 == 2^32
N_PAD = [1, 512, 171798528, 171798529, EDGE - 512, EDGE - 1, EDGE, EDGE + 1, EDGE + 512, 1 << 31, (1 << 32) - 1]
LAYOUT_N = [1, 1000, 171798528, 171798529, EDGE - 1, EDGE]

DRIVER = r'''
#include <cstdio>
#include "photon_plan.hpp"
using namespace mcrat;
int main()
{
    static_assert(photon_addressing(1) == PHOTON_ADDR_BYTE_OFFSET, "usable in a constant expression");
    printf("consts: %d %d %d\n", (int)PHOTON_ADDR_INDEX, (int)PHOTON_ADDR_BYTE_OFFSET, N_BLOCK_COLS);
    const unsigned long long n_pad[] = {@N_PAD@};
    for (unsigned long long n : n_pad) printf("addr_%llu: %d\n", n, (int)photon_addressing((size_t)n));
    const int layout_n[] = {@LAYOUT_N@};
    for (int n : layout_n) {
        PhotonLayout l;
        const PhotonLayoutStatus st = photon_layout(n, &l);
        printf("layout_%d: %d %d %d\n", n, (int)st, st == PHOTON_LAYOUT_OK ? l.n_pad : -1, st == PHOTON_LAYOUT_OK ? (int)photon_addressing((size_t)l.n_pad) : -1);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rule's driver")
    d = tmp_path_factory.mktemp("photon_offset_rule")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER.replace("@N_PAD@", ", ".join("%dull" % n for n in N_PAD)).replace("@LAYOUT_N@", ", ".join(str(n) for n in LAYOUT_N)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    res = {}
    for line in text.splitlines():
        key, _, rest = line.partition(":")
        res[key] = [int(v) for v in rest.split()]
    assert res["consts"] == [INDEX, BYTE_OFFSET, 25]
    return res


def test_byte_offsets_up_to_the_last_slot_whose_offset_fits(out):
    for n in N_PAD:
        assert out["addr_%d" % n] == [BYTE_OFFSET if n * 8 < 1 << 32 else INDEX], n
    # one slot on either side of n_pad * 8 == 2^32
    assert out["addr_%d" % (EDGE - 1)] == [BYTE_OFFSET]
    assert out["addr_%d" % EDGE] == [INDEX] and out["addr_%d" % (EDGE + 1)] == [INDEX]


def test_a_refused_block_keeps_the_index_accessor(out):
    """what the rule refuses resolves to PHOTON_ADDR_INDEX, the name of the accessor from before byte offsets, at every size up to 2^32 - 1.  Only the
    rule's value is checked here: no kernel with that accessor is built (photon_layout refuses such a block before the rule is asked, next test), and
    a launch handed one returns an error"""
    refused = [n for n in N_PAD if n * 8 >= 1 << 32]
    assert len(refused) >= 4
    assert all(out["addr_%d" % n] == [INDEX] for n in refused)


def test_every_block_the_layout_accepts_has_byte_offsets(out):
    """photon_layout's bound (25 x n_pad < 2^32) is the tighter one: what it lays out has byte offsets, what has none it had refused already"""
    for n in LAYOUT_N:
        status, n_pad, addressing = out["layout_%d" % n]
        if n <= 171798528:
            assert status == 0 and n_pad >= n and n_pad % 512 == 0 and addressing == BYTE_OFFSET, n
        else:
            assert status != 0, n
