"""The table of the developer timelines (covid19uk_amd/csrc/stamps.h: families, word formulas, extents, reset pattern, the
stamped builds) compiled as plain C++ in a small host driver -- seconds, no GPU.  For B in {1, 2, 3, 8} the highest word any
site of a sampler family can form under its guards (slot < 27, step < 12, tix < 1024, the two probe tiles, the two probe
roles) lies inside the family's extent, the extent inside what the host allocates, and the regions of one family do not
meet.  B = 1 is where the PAIR stamps used to run past their buffer, B = 2 where k_leap's role probes used to share the
tile probes' blocks.  The reset pattern has ~0 exactly on the table's min-words; tools/dev/build_variant.sh and
tools/dev/stamps.py state the same builds and the same layout as the header."""
import importlib.util
import os
import subprocess

import pytest

import __graft_entry__ as entry

DRIVER = r"""
#include <cstdio>
#include <initializer_list>
#include "stamps.h"
using namespace seir::stamps;
int main() {
    for (int i = 0; i < NVARIANTS; ++i) std::printf("variant %s|%s|%d|%s\n", VARIANTS[i].tag, VARIANTS[i].flags, (int)VARIANTS[i].family, VARIANTS[i].tool);
    std::printf("family seir %d pair %d leap %d tail %d se %d eval %d\n", F_SEIR, F_PAIR, F_LEAP, F_TAIL, F_SE, F_EVAL);
    for (int B : {1, 2, 3, 8}) {
        std::printf("B %d buffer %zu\n", B, buffer_words(B));
        std::printf("extent %d seir %zu pair %zu leap %zu tail %zu\n", B, extent(F_SEIR, B), extent(F_PAIR, B), extent(F_LEAP, B), extent(F_TAIL, B));
        // the highest word of every kind of site, under the guards of its macro
        std::printf("top %d pair %zu\n", B, pair_word(PAIR_SLOTS - 1, PAIR_STEPS - 1, PAIR_NW - 1));
        std::printf("top %d leap_chain %zu\n", B, leap_chain_word(B - 1, 15, 7));
        std::printf("top %d leap_tile %zu\n", B, leap_tile_word(B, 1, 15, 7));
        std::printf("top %d leap_role %zu\n", B, leap_role_word(B, 1, 15, 15));
        std::printf("top %d leap_all %zu\n", B, leap_all_word(B, LEAP_ALL_TILES - 1, 3));
        std::printf("top %d tail %zu\n", B, tail_word(B - 1, TAIL_NW - 1));
        std::printf("top %d seir %d\n", B, (SW_DELTA + 3 > SW_ROLE + 3 ? SW_DELTA : SW_ROLE) + 3);
        // the lowest word of every region of LEAP (they must not meet)
        std::printf("low %d leap %zu %zu %zu %zu\n", B, leap_chain_word(0, 0, 0), leap_tile_word(B, 0, 0, 0), leap_role_word(B, 0, 0, 0), leap_all_word(B, 0, 0));
        for (Family f : {F_SEIR, F_PAIR, F_LEAP, F_TAIL}) {
            std::printf("min %d %d", B, (int)f);
            for (size_t w = 0; w < extent(f, B); ++w) if (min_word(f, B, w)) std::printf(" %zu", w);
            std::printf("\n");
        }
    }
}
"""
BS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        hipcc = entry._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("stamps_table")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    t = {"variants": [], "top": {}, "low": {}, "min": {}, "extent": {}, "buffer": {}}
    for ln in out:
        k, rest = ln.split(" ", 1)
        if k == "variant":
            t["variants"].append(rest.split("|"))
        elif k == "family":
            w = rest.split()
            t["family"] = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
        elif k == "B":
            w = rest.split()
            t["buffer"][int(w[0])] = int(w[2])
        elif k == "extent":
            w = rest.split()
            t["extent"][int(w[0])] = {w[i]: int(w[i + 1]) for i in range(1, len(w), 2)}
        elif k == "top":
            B, name, v = rest.split()
            t["top"][(int(B), name)] = int(v)
        elif k == "low":
            w = rest.split()
            t["low"][int(w[0])] = [int(x) for x in w[2:]]
        elif k == "min":
            w = [int(x) for x in rest.split()]
            t["min"][(w[0], w[1])] = set(w[2:])
    return t


def _tools_stamps():
    spec = importlib.util.spec_from_file_location("dev_stamps", os.path.join(entry.ROOT, "tools", "dev", "stamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("B", BS)
def test_every_site_lies_inside_its_family_and_the_family_inside_the_buffer(table, B):
    ext = table["extent"][B]
    fam = {"pair": "pair", "leap_chain": "leap", "leap_tile": "leap", "leap_role": "leap", "leap_all": "leap", "tail": "tail",
           "seir": "seir"}
    for site, f in fam.items():
        assert table["top"][(B, site)] < ext[f], (B, site)
    for f in ("seir", "pair", "leap", "tail"):
        assert ext[f] <= table["buffer"][B], (B, f)
    # what the earlier code allocated whatever the family: at least as much now
    assert table["buffer"][B] >= (B + 2) * 128 + 4096


@pytest.mark.parametrize("B", BS)
def test_the_regions_of_k_leap_do_not_meet(table, B):
    lo = table["low"][B]
    top = [table["top"][(B, s)] for s in ("leap_chain", "leap_tile", "leap_role", "leap_all")]
    assert lo[0] == 0
    for k in range(3):
        assert top[k] < lo[k + 1], (B, k)


@pytest.mark.parametrize("B", BS)
def test_the_reset_pattern_has_all_ones_exactly_on_the_min_words(table, B):
    f = table["family"]
    assert table["min"][(B, f["seir"])] == set() and table["min"][(B, f["pair"])] == set()
    # TAIL: first tile start, first role past its wait, first role start -- of every chain
    assert table["min"][(B, f["tail"])] == {b * 8 + k for b in range(B) for k in (0, 2, 5)}
    # LEAP: the even words of the chains' blocks (min over the workgroups), nothing behind them
    assert table["min"][(B, f["leap"])] == {w for w in range(B * 128) if w % 2 == 0}


def test_build_variant_sh_states_the_header_s_builds(table):
    listed = subprocess.run(["bash", os.path.join(entry.ROOT, "tools", "dev", "build_variant.sh"), "--list"], check=True,
                            capture_output=True, text=True).stdout.splitlines()
    assert [ln.split("|") for ln in listed] == [v[:2] for v in table["variants"]]
    assert len(listed) >= 8
    for tag, flags, family, tool in table["variants"]:
        assert os.path.exists(os.path.join(entry.ROOT, tool)), tool
        on = [w for w in flags.split() if w.startswith("-D") and w.split("=")[0].endswith("_STAMPS")]
        assert len(on) == 1, f"{tag}: one family per build"


@pytest.mark.parametrize("B", BS)
def test_the_tools_layout_is_the_header_s(table, B):
    st = _tools_stamps()
    ext = table["extent"][B]
    for f in ("seir", "pair", "leap", "tail"):
        assert st.extent(f, B) == ext[f], f
    leap = st.LAYOUT["leap"](B)
    assert [leap[k][0] for k in ("chains", "tiles", "roles", "all")] == table["low"][B]
    assert st.LAYOUT["pair"](B)["steps"][1] == (27, 12, 16) and table["top"][(B, "pair")] == 27 * 12 * 16 - 1
