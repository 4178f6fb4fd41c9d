"""Two pieces of index arithmetic that left the event-update kernels' steps, against the divisions they replace, without
a GPU (a small host driver around the headers, compiled as plain C++):

  * covid19uk_amd/csrc/move_cells.h, cell_row<MM>: the updated row of a cell of an E->I-type proposal's own-rows
    enumeration (own_rows_delta) as a count of compares -- equal to cell / total_w for every n <= MM updated rows, every
    total_w in 1 .. 2 x 128 days of windows and every cell < n * total_w, for both instance bounds (MM_SMALL, MMAX);
  * covid19uk_amd/csrc/sweep_plan.h, band_rows: the rows per band workgroup the pair launches now take as
    an argument -- equal to the expression pair_step, pair_band_block and pair_band_finish divided out in every step,
    (M + nband - 1) / nband, at the M that turn the band's shape and for every nband the plan can return there."""
import subprocess

import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib
from tests import test_sweep_plan as P

DRIVER = r"""
#include <cstdio>
#include "move_cells.h"
#include "sweep_plan.h"
template <int MM>
static long check(long &cells) {
    long bad = 0;
    for (int n = 1; n <= MM; ++n)
        for (int total_w = 1; total_w <= 2 * 128; ++total_w)
            for (int cell = 0; cell < n * total_w; ++cell, ++cells)
                bad += seir::cell_row<MM>(cell, total_w, n) != cell / total_w;
    return bad;
}
int main() {
    static_assert(seir::plan::MM_SMALL == 2 && seir::plan::MMAX == 4, "the two instance bounds");
    long c2 = 0, c4 = 0;
    const long b2 = check<seir::plan::MM_SMALL>(c2), b4 = check<seir::plan::MMAX>(c4);
    std::printf("%ld %ld %ld %ld\n", b2, c2, b4, c4);
    seir::SweepInputs in;
    int xl, og, ug, pl;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &in.M, &in.Mp, &in.Tp, &in.ntc, &in.nmt,
                      &in.nrb_d, &in.nb, &in.L, &in.n_scans, &in.record_events, &in.hmc_mode, &in.moves_mode, &in.leap_rows,
                      &xl, &og, &ug, &in.affinity, &in.cus, &in.leap_occ24, &in.leap_occ32, &pl) == 21) {
        in.xcd_local = xl; in.one_group = og; in.use_graph = ug; in.pairs_lds = pl;
        const seir::SweepPlan p = seir::plan_sweep(in);
        std::printf("%d %d\n", p.nband, seir::band_rows(in.M, p.nband));
    }
}
"""
ROWS_M = (1, 11, 17, 380, 512, 513, 2048)
MVW = 8                                               # waves of a band workgroup (moves_kernel.h)
# what moves plan_sweep's choice of nband: the chains (16-row band workgroups, 32-row ones, none), the launch form, where
# the chains sit, a chip too small for any band
CHAINS = (1, 3, 8, 16, 24, 32, 64)
FORMS = (dict(), dict(moves_mode=4), dict(moves_mode=3), dict(moves_mode=2), dict(moves_mode=1), dict(xcd_local=0), dict(cus=16),
         dict(cus=304))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    try:
        hipcc = entry._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("move_cells")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(lines=()):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), check=True, capture_output=True,
                             text=True).stdout.strip().split("\n")
        return [int(v) for v in out[0].split()], [tuple(int(v) for v in l.split()) for l in out[1:]]
    return run


def test_the_bounds_are_the_librarys():
    assert (_lib.MM_SMALL, _lib.MMAX) == (2, 4)


def test_cell_row_is_the_quotient_for_every_cell_of_both_instance_bounds(driver):
    (bad2, cells2, bad4, cells4), _ = driver()
    # every (n, total_w, cell) was visited: sum over n <= MM and total_w <= 256 of n total_w cells
    want = lambda mm: sum(n * w for n in range(1, mm + 1) for w in range(1, 257))
    assert (cells2, cells4) == (want(2), want(4))
    assert (bad2, bad4) == (0, 0)


@pytest.mark.parametrize("M", ROWS_M)
def test_the_hosts_rows_per_band_workgroup_are_the_kernels_old_expression(driver, M):
    lines = [P.inputs(f"slow_{M}x64", nb=nb, **kw) for nb in CHAINS for kw in FORMS]
    _, rows = driver(lines)
    assert len(rows) == len(lines)
    seen = {}
    for nband, rpb in rows:
        old = (M + nband - 1) // nband if nband else 0       # pair_step / pair_band_block / pair_band_finish, up to round 34
        assert rpb == old, (M, nband, rpb, old)
        assert (rpb > 2 * MVW) == (old > 2 * MVW)            # the band's shape: two or four rows per wave
        seen[nband] = rpb
    print(M, seen)
    # the plan returned every kind there is for the size: no band, and (where a band fits a chip at all) 16-row workgroups
    assert 0 in seen and (M > 2000 or (M + 15) // 16 in seen), seen
    if M == 380:
        assert seen == {0: 0, 24: 16, 12: 32}
