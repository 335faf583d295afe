"""The halving schedule of a group's log-likelihood sums (csrc/ekf_wave.h: wave_halving_tree_sums) against the xor-butterfly
it replaces (wave_xor_tree_sum for each of the G particles), emulated lane by lane on numpy float32 and compared as bit
patterns.

The butterfly: every lane holds a value of every particle, t[k][j] <- t[k][j] + t[k][j ^ s] for s = 1 .. 32, and lane k keeps
t[k][k].  The halving schedule: at the step of bit b (s = 1 << b), while more than one particle is left in a lane, lane j keeps
of every pair of neighbouring values the one whose particle has bit b as j has it and sends the other to lane j ^ s, which keeps
exactly that one; so the lane adds what the butterfly adds for the particles it keeps — own value first, the partner's second —
and after log2 G such steps holds ONE particle, j & (G - 1), on which the remaining steps run as in the butterfly.  Lane k < G
ends with particle k's total, made by the same additions on the same operands in the same order as the butterfly makes in
lane k: the same bits, NaN payloads included.
"""
import numpy as np
import pytest

from conftest import bits

LANES = 64
J = np.arange(LANES)


def butterfly(t):
    """t: [G][64] float32 -> [G][64], every lane the tree sum t[j] + t[j ^ s], s = 1 .. 32"""
    t = t.copy()
    s = 1
    while s < LANES:
        t = t + t[:, J ^ s]
        s <<= 1
    return t


def halving(t, swap_at=None, skip=None):
    """the device function statement by statement: v[i] = (up ? v[2i+1] : v[2i]) + shfl_xor(up ? v[2i] : v[2i+1], s) while
    values are left to halve, then v[0] = v[0] + shfl_xor(v[0], s).  swap_at / skip: the two mistakes the test must catch —
    the halves assigned the other way round at that step, that step left out."""
    v = [row.copy() for row in t]
    m, s = len(v), 1
    while s < LANES:
        if s == skip:
            if m > 1:
                v, m = v[0:m:2], m // 2
            s <<= 1
            continue
        if m > 1:
            up = (J & s) != 0
            if s == swap_at:
                up = ~up
            nxt = []
            for i in range(m // 2):
                keep = np.where(up, v[2 * i + 1], v[2 * i])
                send = np.where(up, v[2 * i], v[2 * i + 1])
                nxt.append(keep + send[J ^ s])
            v, m = nxt, m // 2
        else:
            v = [v[0] + v[0][J ^ s]]
        s <<= 1
    return v[0]


def _values(rng, kind, shape):
    f32 = np.float32
    if kind == "normal":
        return rng.standard_normal(shape).astype(f32) * f32(37.0)
    if kind == "loglik":          # what the kernel sums: negative terms of a few units to a few thousand
        return -(rng.random(shape).astype(f32) * f32(3000.0)) - f32(1.8378770664)
    if kind == "mixed_scale":     # huge and tiny side by side: every addition rounds
        return (rng.standard_normal(shape) * 10.0 ** rng.integers(-30, 31, shape)).astype(f32)
    if kind == "denormal":
        return (rng.integers(-(1 << 22), 1 << 22, shape).astype(np.int64) * 2.0 ** -149).astype(f32)
    if kind == "zeros":           # +0 and -0, a few denormals among them
        z = np.where(rng.random(shape) < 0.5, f32(0.0), f32(-0.0)).astype(f32)
        d = rng.random(shape) < 0.1
        z[d] = (rng.integers(-3, 4, int(d.sum())) * 2.0 ** -149).astype(f32)
        return z
    if kind == "overflow":        # sums that reach an infinity on the way, and inf - inf
        return (rng.choice([3.0e38, -3.0e38, 1.0e37, -1.0, 1.0e-40], shape)).astype(f32)
    if kind == "special":         # infinities and NaNs with payloads of their own among ordinary values
        a = rng.standard_normal(shape).astype(f32)
        u = a.view(np.uint32)
        r = rng.random(shape)
        a[r < 0.04] = np.inf
        a[(r >= 0.04) & (r < 0.08)] = -np.inf
        nan = (r >= 0.08) & (r < 0.14)
        u[nan] = 0x7FC00000 | rng.integers(0, 1 << 22, int(nan.sum())).astype(np.uint32) | \
            (rng.integers(0, 2, int(nan.sum())).astype(np.uint32) << 31)
        return a
    raise ValueError(kind)


KINDS = ["normal", "loglik", "mixed_scale", "denormal", "zeros", "overflow", "special"]


def _cases(G, kind, reps=24):
    rng = np.random.default_rng(1000 * G + KINDS.index(kind))
    for nslots in range(1, G + 1):
        for _ in range(reps):
            t = _values(rng, kind, (G, LANES))
            t[nslots:] = np.float32(0.0)   # the accumulators of the slots beyond the group's last particle hold zeros
            yield nslots, t


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G", [2, 4, 8])
def test_halving_schedule_gives_the_butterflys_bits(G, kind):
    with np.errstate(all="ignore"):
        for nslots, t in _cases(G, kind):
            want = butterfly(t)
            got = halving(t)
            # lane k < nslots: particle k's total (what the kernel stores) ...
            k = np.arange(nslots)
            assert np.array_equal(bits(got[k]), bits(want[k, k])), (G, kind, nslots)
            # ... and every lane j that of particle j & (G - 1), as the butterfly leaves it in that lane
            assert np.array_equal(bits(got), bits(want[J & (G - 1), J])), (G, kind, nslots)


@pytest.mark.parametrize("G", [2, 4, 8])
def test_wrong_schedules_are_caught(G):
    """the halves assigned the other way round at any halving step, or any step skipped, changes what lane k < nslots holds"""
    with np.errstate(all="ignore"):
        steps = [1 << b for b in range(6)]
        for nslots in range(1, G + 1):
            rng = np.random.default_rng(77 + G)
            t = _values(rng, "loglik", (G, LANES))
            t[nslots:] = np.float32(0.0)
            want = butterfly(t)
            k = np.arange(nslots)
            assert np.array_equal(bits(halving(t)[k]), bits(want[k, k]))
            for s in steps:
                if s < G and nslots > 1:   # (with one particle and zeros in the other slots lane 0 may be handed a zero row)
                    assert not np.array_equal(bits(halving(t, swap_at=s)[k]), bits(want[k, k])), (G, nslots, "swap", s)
                assert not np.array_equal(bits(halving(t, skip=s)[k]), bits(want[k, k])), (G, nslots, "skip", s)
