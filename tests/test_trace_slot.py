"""The thinning rule (covid19uk_amd/csrc/trace_slot.h: trace_slot0 / trace_slot, the one definition every trace writer of
the kernels calls) compiled as plain C++ in a small host driver -- seconds, no GPU.  After a trace reset sweep i = 0, 1, ...
is recorded iff (i + 1) % k == 0, in slot first_slot + i // k (tfp.mcmc.sample_chain(num_steps_between_results = k - 1));
k = 1 is `sweep - slot0`, as before thinning existed, for every input."""
import subprocess

import pytest

import __graft_entry__ as entry

DRIVER = r"""
#include <cstdio>
#include "trace_slot.h"
int main() {
    unsigned op, a, b, k, cap;
    // 0 sweep first k _  -> trace_slot0(sweep, first, k);   1 sweep slot0 k cap -> trace_slot(sweep, slot0, k, cap)
    while (std::scanf("%u %u %u %u %u", &op, &a, &b, &k, &cap) == 5)
        std::printf("%u\n", op == 0 ? seir::trace_slot0(a, b, k) : seir::trace_slot(a, b, k, cap));
}
"""
W = 2 ** 32


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    try:
        hipcc = entry._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("trace_slot")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(rows):
        text = "".join(" ".join(str(int(x) % W) for x in r) + "\n" for r in rows)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split()
        assert len(out) == len(rows)
        return [int(x) for x in out]
    return run


CAP = 16


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("k", [1, 2, 3, 7, 20])
@pytest.mark.parametrize("start", [0, 1000, 12345678])
def test_sweep_i_is_recorded_iff_it_closes_a_group_of_k(helper, k, first, start):
    slot0, = helper([(0, start, first, k, 0)])
    n = 3 * k + 1                                               # sweeps 0 ... 3k after the reset
    got = helper([(1, start + i, slot0, k, CAP) for i in range(n)])
    kept = 0
    for i, g in enumerate(got):
        if (i + 1) % k == 0 and first + i // k < CAP:
            assert g == first + i // k, (i, g)
            kept += 1
        else:
            assert g >= CAP, f"sweep {i} must not be recorded, got slot {g}"
    assert kept == (n // k if k > 1 or first == 0 else min(n, CAP - first))
    # run(n * k) fills exactly n slots and the last recorded draw is the last sweep
    assert got[3 * k - 1] == first + 2 if k > 1 else True


@pytest.mark.parametrize("k", [1, 2, 3, 7, 20])
def test_a_slot_at_or_beyond_the_capacity_is_not_recorded(helper, k):
    cap, first = 4, 2
    slot0, = helper([(0, 50, first, k, 0)])
    got = helper([(1, 50 + i, slot0, k, cap) for i in range(6 * k)])
    for i, g in enumerate(got):
        want = first + i // k
        if (i + 1) % k == 0 and want < cap:
            assert g == want
        else:
            assert g >= cap, (i, g)


@pytest.mark.parametrize("start", [0, 7, W - 3, W - 1])
@pytest.mark.parametrize("first", [0, 5])
def test_thin_1_is_sweep_minus_slot0_for_every_input(helper, start, first):
    """Today's behaviour, wrap of the 32-bit sweep counter included."""
    slot0, = helper([(0, start, first, 1, 0)])
    assert slot0 == (start - first) % W
    sweeps = [start + i for i in range(8)] + [start - 1, start + W // 2, 0, W - 1]
    for cap in (1, 16, 2 ** 31 - 1):
        got = helper([(1, s, slot0, 1, cap) for s in sweeps])
        assert got == [(s - slot0) % W for s in sweeps]
    # k = 0 (an all-zero descriptor tail) means the same
    assert helper([(1, s, slot0, 0, 16) for s in sweeps]) == [(s - slot0) % W for s in sweeps]
    assert helper([(0, start, first, 0, 0)]) == [slot0]


@pytest.mark.parametrize("k", [2, 4, 16])
def test_powers_of_two_are_exact_across_the_wrap(helper, k):
    first, start = 3, W - 5
    slot0, = helper([(0, start, first, k, 0)])
    got = helper([(1, start + i, slot0, k, CAP) for i in range(3 * k)])
    for i, g in enumerate(got):
        if (i + 1) % k == 0:
            assert g == first + i // k
        else:
            assert g >= CAP


def test_every_trace_writer_goes_through_the_helper():
    """No kernel is left on the old expression: Chains::slot0 is read by chain_trace_slot and written by k_set_slot0 only."""
    import os
    import re
    for name in ("sampler_kernels.h", "moves_kernel.h"):
        text = open(os.path.join(entry.CSRC, name)).read()
        text = re.sub(r"//[^\n]*", "", text)
        uses = [ln.strip() for ln in text.splitlines() if "slot0" in ln]
        for ln in uses:
            assert ("unsigned *slot0" in ln or "trace_slot(sweep, ch.slot0[0]" in ln or "trace_slot0(ch.sweep[0]" in ln), ln
