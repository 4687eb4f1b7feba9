"""Plan selection against a recorded table (tests/golden/plan_table.json):
which algorithm build_plan takes for a length, and with which split, radix
list and convolution length, does not change when the planner's code moves.
No transform runs; the plans are built under ALGO_NO_RACE, where the choice
does not depend on a timing."""
import importlib
import json
import math
import os

import pytest

from conftest import GOLDEN

# (n, forced chirp-z). By the recorded table: kind 0: 0, 1; 1: 2, 4096;
# 2: 2^16, 2^21; 3: 8191 and the forced 4096 (a power-of-2 M), 2062, 3067
# and the forced 3000 (the M = 16 RB 16 kernel), 4099 (M = 16 R1 R2 16 = 9216),
# 2729 and 5209 (the smooth-L kernel, L = 5760 and 10800), 8209 and 10007
# (output parts); 4: the forced 10000, 16411; 5: 3000, 5000 (compiled lists),
# 5400 (runtime-compiled); 6: 10000 (rows of 16), 44100, 30000, 10^6 (smooth
# rows), 64 * 8209, 2 * 10007, 64 * 8191 (three passes); 7: 131, 3001, 6007;
# 8: 4097, 3027.
# No length gives kind 4 a convolution length that is no power of 2:
# build_plan looks for a smooth M only where M <= 65536 has no two-pass
# four-step (2^15 .. 2^20), and a composed chirp-z has M >= 2^15.
LENGTHS = [(0, False), (1, False), (2, False), (4096, False), (1 << 16, False), (1 << 21, False),
           (3000, True), (4096, True), (10000, True),
           (3000, False), (5000, False), (5400, False),
           (10000, False), (44100, False), (30000, False), (10 ** 6, False),
           (64 * 8209, False), (2 * 10007, False), (64 * 8191, False),
           (2062, False), (3067, False), (8209, False), (16411, False),
           (131, False), (3001, False), (6007, False),
           (2729, False), (8191, False),
           (4097, False), (3027, False),
           (4099, False), (5209, False), (10007, False)]
TABLE = os.path.join(GOLDEN, "plan_table.json")


def key(n, chirpz):
    return f"{n}{'/chirpz' if chirpz else ''}"


def record(D, n, chirpz):
    """The plan for n as the C ABI reports it (gdsp_plan_kind, _parts, _info,
    _radices), built now: not through device.plan's cache."""
    p = D.Plan(n, chirpz)
    return {"kind": p.kind, "parts": p.parts, "m": p.m, "n1": p.n1, "n2": p.n2,
            "runtime_compiled": int(p.runtime_compiled), "radices": list(p.radices)}


def build_table():
    D = importlib.import_module("go-dsp_amd.device")
    F = importlib.import_module("go-dsp_amd.fft")
    before = F.Algorithm()
    F.SetAlgorithm(F.ALGO_NO_RACE)
    try:
        return {key(n, c): record(D, n, c) for n, c in LENGTHS}
    finally:
        F.SetAlgorithm(before)


def test_table_covers_every_branch():
    """The recorded table itself: every kind, an output-split chirp-z, both
    compiled and runtime-compiled plans, and the kind-3 convolution lengths
    that are no power of 2: the M = 16 RB 16 kernel's (<= 6144, compiled) and
    the smooth-L kernel's (> 6144, runtime-compiled, L the product of its
    radix list). (Kind 4 with such a length: no length has it, see above.)"""
    with open(TABLE) as f:
        rec = json.load(f)["plans"]
    assert len(LENGTHS) <= 40 and set(rec) == {key(n, c) for n, c in LENGTHS}
    rows = list(rec.values())
    pow2 = lambda m: m & (m - 1) == 0
    prod = lambda rad: math.prod(rad) if rad else 0
    assert {r["kind"] for r in rows} == set(range(9))
    assert any(r["parts"] > 1 for r in rows)
    assert {r["runtime_compiled"] for r in rows} == {0, 1}
    k3 = [r for r in rows if r["kind"] == 3 and not pow2(r["m"])]
    assert any(r["m"] <= 6144 and not r["runtime_compiled"] for r in k3)
    assert any(r["m"] > 6144 and r["runtime_compiled"] and prod(r["radices"]) == r["m"] for r in k3)


@pytest.mark.gpu
def test_plan_table_unchanged(gdsp):
    with open(TABLE) as f:
        rec = json.load(f)["plans"]
    got = build_table()
    diff = {k: (got[k], rec[k]) for k in rec if got[k] != rec[k]}
    assert not diff, diff
