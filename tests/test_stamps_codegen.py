"""The stamp macros of covid19uk_amd/csrc/stamps.h cost the default build nothing, and a stamped build one clock read per
site at the table's words.  A small device unit on the header -- a kernel that uses the plain, drained, min and max forms
and hands the stamp contexts to a __forceinline__ callee -- is compiled to gfx950 assembly: with no family on it is,
instruction for instruction, the same kernel written without the macros and reads no clock; with a family on, every site
of that family reads the clock once and its store or atomic lands at the word the table gives.  Seconds, no GPU."""
import importlib.util
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

# lines that end in `// stamp` exist only in the stamped form of the unit
UNIT = r"""
#include "stamps.h"
namespace seir {
struct Chains { double *hs; unsigned long long *stamps; };
struct SamplerCfg { int B; };
struct MvLds : MoveStamp { int *rg; };
__device__ __forceinline__ int callee(const Chains &ch, const MvLds &L, PairStamp qst, RoleStamp probe, int v) {
    MSTAMP(L, 5);                                            // stamp
    QSTAMP(qst, 3);                                          // stamp
    v = v * 3 + 1;
    CPROBE(probe, 9);                                        // stamp
    return v;
}
template <int STAGE>
__global__ void k_unit(Chains ch, SamplerCfg s, int *out, int b, int par, int it) {
    STAMP(0);                                                // stamp
    int v = out[threadIdx.x];
    STAMP_DRAIN(10);                                         // stamp
    MvLds L{};
    L.rg = out;
    const MoveStamp mst = MOVE_STAMP_CTX(b == 0 && par == 1);   // stamp
    MOVE_STAMP_PASS(L, mst);                                 // stamp
    const PairStamp qst = PAIR_STAMP_CTX(b, 2, 3);
    TSTAMP_MIN(1, 0);                                        // stamp
    v = callee(ch, L, qst, RoleStamp{nullptr}, v);
    TSTAMP_MINMAX(1, 2, 3);                                  // stamp
    L.rg[threadIdx.x] = v;
    QSTAMP_T(qst, threadIdx.x == 64, 7);                     // stamp
    TSTAMP_MAX_DRAINED(1, 4);                                // stamp
    if (threadIdx.x == 0) { LSTAMP_MIN(2); LSTAMP_MAX(3); }  // stamp
}
template __global__ void k_unit<2>(Chains, SamplerCfg, int *, int, int, int);
}
"""


def _compile(d, name, text, flags=()):
    src, out = d / f"{name}.hip", d / f"{name}.s"
    src.write_text(text)
    subprocess.run([entry._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", entry.CSRC,
                    *flags, "-o", str(out), str(src)], check=True, capture_output=True, text=True)
    lines = [l.split(";")[0].strip() for l in out.read_text().splitlines()]
    return [l for l in lines if l and not l.startswith((".", "//")) and not l.endswith(":")]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        entry._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("stamps")
    # ... and the one context the callee's signature carries is spelled out as the empty type it is
    bare = "\n".join(l for l in UNIT.splitlines() if not l.rstrip().endswith("// stamp")).replace("PAIR_STAMP_CTX(b, 2, 3)", "PairStamp{}")
    assert "STAMP" not in bare.replace("MoveStamp", "").replace("PairStamp", "").replace("RoleStamp", "")
    return {"bare": _compile(d, "bare", bare), "off": _compile(d, "off", UNIT),
            "seir": _compile(d, "seir", UNIT, ["-DSEIR_STAMPS"]), "pair": _compile(d, "pair", UNIT, ["-DPAIR_STAMPS=1"]),
            "tail": _compile(d, "tail", UNIT, ["-DTAIL_STAMPS"]), "leap": _compile(d, "leap", UNIT, ["-DLEAP_STAMPS=2"])}


def _layout():
    spec = importlib.util.spec_from_file_location("dev_stamps", os.path.join(entry.ROOT, "tools", "dev", "stamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _clock_reads(lines):
    return sum(l.startswith("s_memrealtime") for l in lines)


def _offsets(lines, prefix):
    """byte offsets of the unit's accesses of that kind (the stamp region's base is a kernel argument: the word is the offset)"""
    out = []
    for l in lines:
        if l.startswith(prefix):
            m = re.search(r"offset:(\d+)", l)
            out.append(int(m.group(1)) if m else 0)
    return sorted(out)


def test_no_family_on_the_macros_are_no_code(asm):
    assert asm["off"] == asm["bare"]
    assert _clock_reads(asm["off"]) == 0
    assert len(asm["off"]) > 5, "the kernel itself is there"


def test_seir_plain_and_drained_stores_at_their_words(asm):
    a = asm["seir"]
    assert _clock_reads(a) == 3                                  # STAMP, STAMP_DRAIN, MSTAMP through the callee
    # the kernel's own store of v is a dword; the stamps are the 64-bit stores: words 0, 10 and 5
    assert _offsets(a, "global_store_dwordx2") == [0 * 8, 5 * 8, 10 * 8]
    drain = [i for i, l in enumerate(a) if l.startswith("s_waitcnt") and "vmcnt(0)" in l and "lgkmcnt(0)" in l]
    clocks = [i for i, l in enumerate(a) if l.startswith("s_memrealtime")]
    assert any(d < c for d in drain for c in clocks[1:]), "STAMP_DRAIN waits for everything before it reads the clock"


def test_pair_context_reaches_the_callee_and_words_follow_the_table(asm):
    a = asm["pair"]
    assert _clock_reads(a) == 2                                  # QSTAMP in the callee, QSTAMP_T by another thread
    nslot, nstep, nw = _layout().LAYOUT["pair"](8)["steps"][1]
    word = lambda slot, step, i: (slot * nstep + step) * nw + i
    assert _offsets(a, "global_store_dwordx2") == [word(2, 3, 3) * 8, word(2, 3, 7) * 8]


def test_tail_min_max_and_drained_atomics(asm):
    a = asm["tail"]
    assert _clock_reads(a) == 3                                  # MIN, MINMAX (one reading for two words), MAX_DRAINED
    assert _offsets(a, "global_atomic_umin_x2") == [(1 * 8 + 0) * 8, (1 * 8 + 2) * 8]
    assert _offsets(a, "global_atomic_umax_x2") == [(1 * 8 + 3) * 8, (1 * 8 + 4) * 8]
    assert not any(l.startswith("global_store_dwordx2") for l in a)


def test_leap_level_2_min_and_max_of_the_chain_s_words(asm):
    a = asm["leap"]
    assert _clock_reads(a) == 2                                  # LSTAMP_MIN, LSTAMP_MAX; the role's context was null
    assert len(_offsets(a, "global_atomic_umin_x2")) == 1 and len(_offsets(a, "global_atomic_umax_x2")) == 1
