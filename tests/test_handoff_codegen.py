"""The hand-off words of covid19uk_amd/csrc/handoff.h stay single 16-byte accesses.  A word {a, seq, b, seq} is only safe
because each 8-byte half lands whole and the consumer looks at both: every store of a word must be ONE global_store_dwordx4
(with the s_nop 1 that gfx950 needs behind it before its data registers are written again), never two narrower stores, and
every load of a word one global_load_dwordx4 past the L1 (sc1).  A small device unit built on the header is compiled to
gfx950 assembly -- seconds, no GPU."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

UNIT = r"""
#include "handoff.h"
__global__ void store_double(uint4 *p, const double *v, unsigned seq) { ll_store(p + threadIdx.x, v[threadIdx.x], seq); }
__global__ void store_dwords(uint4 *p, const int *src, unsigned seq) { move_store_ll<59>(p, src, (int)(threadIdx.x & 63), seq); }
__global__ void poll_doubles(const uint4 *in, uint4 *out, unsigned seq, unsigned *late) {
    const uint4 *p[6] = {in + threadIdx.x, in + 64 + threadIdx.x, in + 128, in + 192 + threadIdx.x, in + 256, in + 320};
    double v[6];
    ll_poll<6>(p, seq, late, v);
    ll_store(out + threadIdx.x, v[0] + v[1] + v[2] + v[3] + v[4] + v[5], seq);
}
__global__ void poll_dwords(const uint4 *in, uint4 *out, unsigned seq, unsigned *late) {
    __shared__ int d[59];
    if (threadIdx.x < 64) move_wait_ll<59>(d, in, (int)threadIdx.x, seq, late);
    __syncthreads();
    ll_store(out + threadIdx.x, (double)d[threadIdx.x % 59], seq);
}
"""


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = entry._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("handoff")
    src, out = d / "unit.hip", d / "unit.s"
    src.write_text(UNIT)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", entry.CSRC,
                    "-o", str(out), str(src)], check=True, capture_output=True, text=True)
    lines = [l.split(";")[0].strip() for l in out.read_text().splitlines()]
    return [l for l in lines if l and not l.startswith((".", "//")) and not l.endswith(":")]


def test_every_word_store_is_one_dwordx4_followed_by_s_nop(asm):
    sites = [i for i, l in enumerate(asm) if l.startswith("global_store_dwordx4")]
    assert len(sites) >= 4, "one store site per kernel of the unit"
    for i in sites:
        assert asm[i + 1].startswith("s_nop"), asm[i:i + 2]


def test_no_narrower_global_store(asm):
    # every global store of the unit is a word store: none may be split into dword / dwordx2 / dwordx3 pieces
    narrow = [l for l in asm if re.match(r"global_store_(dword|dwordx2|dwordx3|short|byte)\b", l)]
    assert not narrow, narrow


def test_every_word_load_reads_past_the_l1(asm):
    loads = [l for l in asm if l.startswith("global_load_dwordx4")]
    assert len(loads) >= 7, "six words in poll_doubles, one in poll_dwords"
    assert all(re.search(r"\bsc1\b", l) for l in loads), loads
