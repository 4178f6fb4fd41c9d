"""The hand-off words by which k_move_pairs' band workgroups leave their partial sums for the roles of the next step
(covid19uk_amd/csrc/handoff.h: pair_sums_store / pair_sums_wait) stay single 16-byte accesses, like every other word of
the header (tests/test_handoff_codegen.py): a store is ONE global_store_dwordx4 with the s_nop gfx950 needs behind it, a
load one global_load_dwordx4 past the L1 (sc1), and nothing narrower is stored.  A small device unit built on the header
is compiled to gfx950 assembly -- seconds, no GPU."""
import re
import subprocess

import pytest

import __graft_entry__ as entry

UNIT = r"""
#include "handoff.h"
// (the values from registers: the only 16-byte loads of the unit are the words')
__global__ void store_sums(uint4 *p, double a, double b, unsigned seq) {
    pair_sums_store(p + 2 * threadIdx.x, a * (double)threadIdx.x, b + (double)threadIdx.x, seq);
}
__global__ void wait_sums(const uint4 *in, uint4 *out, unsigned seq, unsigned *late, int n) {
    double th, cn;
    pair_sums_wait(in + 2 * min((int)threadIdx.x, n - 1), seq, late, th, cn);
    pair_sums_store(out + 2 * threadIdx.x, th, cn, seq);
}
"""


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = entry._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("pair_handoff")
    src, out = d / "unit.hip", d / "unit.s"
    src.write_text(UNIT)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", entry.CSRC,
                    "-o", str(out), str(src)], check=True, capture_output=True, text=True)
    lines = [l.split(";")[0].strip() for l in out.read_text().splitlines()]
    return [l for l in lines if l and not l.startswith((".", "//")) and not l.endswith(":")]


def test_every_word_store_is_one_dwordx4_followed_by_s_nop(asm):
    sites = [i for i, l in enumerate(asm) if l.startswith("global_store_dwordx4")]
    assert len(sites) >= 4, "two words per kernel of the unit"
    for i in sites:
        assert asm[i + 1].startswith("s_nop"), asm[i:i + 2]


def test_no_narrower_global_store(asm):
    narrow = [l for l in asm if re.match(r"global_store_(dword|dwordx2|dwordx3|short|byte)\b", l)]
    assert not narrow, narrow


def test_every_word_load_reads_past_the_l1(asm):
    loads = [l for l in asm if l.startswith("global_load_dwordx4")]
    assert len(loads) >= 2, "both words of a band workgroup in one look"
    assert all(re.search(r"\bsc1\b", l) for l in loads), loads


def test_both_words_are_loaded_before_the_wait(asm):
    # one round trip per look: the two loads are issued back to back, then one s_waitcnt
    i = next(i for i, l in enumerate(asm) if l.startswith("global_load_dwordx4"))
    assert asm[i + 1].startswith("global_load_dwordx4") and asm[i + 2].startswith("s_waitcnt vmcnt(0)"), asm[i:i + 3]
