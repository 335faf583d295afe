"""The exact quotient of offspring_fill_kernel (csrc/comb_quotient.h: a double-precision proposal settled by 128-bit integer
comparisons) on the host, against Python integers: totals around 2^32, 2^47 and 2^62, numerators one below, at and one above
q * total for q in {0, 1, n - 1, n}, and 10^5 seeded random cases — half of them spread over every size of total and quotient,
half made as the kernel makes them, X = N * C - u - 1 with C <= total and u < total.  The driver is built with the address and
undefined-behaviour sanitizers.
"""
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = next(ROOT.glob("*_amd")) / "csrc"
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def quotients(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("comb_quotient")
    exe = tmp / "comb_quotient_driver"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "comb_quotient_driver.cpp")],
                   check=True)

    def run(cases):
        """cases: (X, d) pairs of Python integers -> the driver's quotients"""
        src, out = tmp / "in.bin", tmp / "out.bin"
        np.array([(x >> 64, x & M64, d) for x, d in cases], np.uint64).tofile(src)
        subprocess.run([str(exe), str(src), str(out)], check=True)
        got = np.fromfile(out, np.uint64)
        assert len(got) == len(cases)
        return [int(v) for v in got]

    return run


def _check(quotients, cases):
    got = quotients(cases)
    bad = [(x, d, g) for (x, d), g in zip(cases, got) if g != x // d]
    assert not bad, f"{len(bad)} of {len(cases)} differ, the first: X = {bad[0][0]}, d = {bad[0][1]}: got {bad[0][2]}, want {bad[0][0] // bad[0][1]}"


def test_quotient_at_the_edges_of_every_multiple(quotients):
    cases = []
    for k in (32, 47, 62):
        for total in {(1 << k) + d for d in (-3, -1, 0, 1, 3)} | {(1 << k) + (1 << (k - 1)) + 1, (1 << (k + 1)) - 1}:
            assert 0 < total < 1 << 63
            for n in (1, 2, 65, 4099, 65536, 524288, 1048576, (1 << 31) - 1):
                for q in (0, 1, n - 1, n):
                    for d in (-1, 0, 1):
                        if q * total + d >= 0:
                            cases.append((q * total + d, total))
    assert len(cases) > 1500
    _check(quotients, cases)


def test_quotient_on_random_cases(quotients):
    rng = random.Random(0x0FF5)
    cases = []
    for _ in range(50000):   # every size of total and of quotient, the remainder anywhere
        total = rng.getrandbits(rng.randint(1, 63)) or 1
        q = rng.getrandbits(rng.randint(0, 31))
        cases.append((q * total + rng.randrange(total), total))
    while len(cases) < 100000:   # as the kernel makes them
        total = rng.getrandbits(rng.randint(20, 63)) or 1
        n = rng.randint(1, (1 << 31) - 1)
        c, u = rng.randint(0, total), rng.randrange(total)
        if n * c > u:
            cases.append((n * c - u - 1, total))
    assert len(cases) == 100000
    _check(quotients, cases)
