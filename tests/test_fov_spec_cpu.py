"""tests/_fov_spec.py by hand: with everything in view it is the parents' rule bit for bit; a point exactly on a bound is in view,
for an ordinary and a wrapping arc; NaN never counts as outside; every landmark due a miss is accounted for exactly once;
slam_fov_bound against the spec; and the host program's --prune-fov refuses a bad EDGE.  No GPU."""
import ctypes
import ctypes.util
import subprocess

import numpy as np
import pytest

import _evidence_spec as E
import _fov_spec as V
import _sight_spec as S
from __graft_entry__ import PKG_DIR, load_package

F = np.float32
HIT, MISS, CMAX, RANGE = 2, 1, 8, 4.0
ANGLES = -2.351831 + 0.004363 * np.arange(1079)


def random_case(seed, n=7, L=21):
    rng = np.random.default_rng(seed)
    mp = (rng.standard_normal((n, 5, L + 3)) * 3).astype(F)
    mp[:, 2][rng.random((n, L + 3)) < 0.3] = -1.0
    mp[0, 0, 0] = np.nan
    x, y, th = ((rng.standard_normal(n)).astype(F) for _ in range(3))
    tab = rng.choice(np.array([0, 1, 2, 255], np.uint8), (n, L + 1))
    ev = rng.integers(0, 4, (n + 2, L + 2)).astype(np.uint8)   # (many that cannot pay a miss)
    anc = rng.integers(0, n + 2, n)
    bx, by = np.abs(rng.standard_normal(200) * 2).astype(F), (rng.standard_normal(200) * 2).astype(F)   # returns in front only
    return mp, x, y, th, tab, ev, anc, S.table(bx, by, 64), L


def test_the_diamond_angle_is_the_bin_rule():
    rng = np.random.default_rng(0)
    x, y = (rng.standard_normal(4000) * 3).astype(F), (rng.standard_normal(4000) * 3).astype(F)
    x[:6], y[:6] = (0, -0.0, np.inf, np.nan, 1.0, 1.0), (0, 0.0, 1.0, 1.0, -1e-45, -0.0)
    p, has = V.diamond(x, y)
    assert p.dtype == np.float32 and not np.isnan(p).any() and np.all((p >= 0) & (p <= 4))
    assert has[:6].tolist() == [False, False, False, False, True, True] and p[4] == 4.0 and p[5] == 0.0
    for bins in (32, 1024):
        j, has_bin = S.bin_of(x, y, bins)
        assert np.array_equal(has, has_bin)
        assert np.array_equal(j, np.where(has, (p * F(bins // 4)).astype(np.int64) & (bins - 1), 0))


def test_everything_in_view_is_the_parents_rule(orc):
    mp, x, y, th, tab, ev, anc, T, L = random_case(4)
    for in_place in (False, True):
        a = None if in_place else anc
        got = V.evidence(mp, x, y, th, a, tab, 2, ev, HIT, MISS, CMAX, RANGE, *V.ALL, T, 0.3, L=L, in_place=in_place)
        want = S.evidence(mp, x, y, th, a, tab, 2, ev, HIT, MISS, CMAX, RANGE, T, 0.3, L=L, in_place=in_place)
        assert all(g.tobytes() == w.tobytes() and g.dtype == w.dtype for g, w in zip(got[:4], want))
        assert want[3].sum() > 0 and want[2][:, 0].sum() > 0 and np.all(got[4] == 0)
        got = V.evidence(mp, x, y, th, a, tab, 2, ev, HIT, MISS, CMAX, RANGE, *V.ALL, L=L, in_place=in_place)
        want = E.evidence(mp, x, y, a, tab, 2, ev, HIT, MISS, CMAX, RANGE, L=L, in_place=in_place)
        assert all(g.tobytes() == w.tobytes() and g.dtype == w.dtype for g, w in zip(got[:3], want))
        assert want[2][:, 0].sum() > 0 and np.all(got[3] == 0) and np.all(got[4] == 0)


def one(zx, zy, lo, hi, c=5, tab=255):
    """One particle at the origin with th = 0 (the sensor frame is the world) and one landmark with evidence c -> (evidence, outside)."""
    mp = np.zeros((1, 5, 1), F)
    mp[0, 0, 0], mp[0, 1, 0], mp[0, 2, 0] = zx, zy, 0.3
    z = np.zeros(1, F)
    _, ev, _, _, out = V.evidence(mp, z, z, z, None, np.array([[tab]], np.uint8), 1, np.array([[c]], np.uint8), HIT, MISS, CMAX, RANGE,
                                  F(lo), F(hi))
    return int(ev[0, 0]), int(out[0])


def test_a_bound_itself_is_in_view(orc):
    """Integer points on the diagonals have p = 0.5, 1.5, 2.5, 3.5 exactly."""
    assert V.diamond(F(1), F(1))[0] == 0.5 and V.diamond(F(-2), F(2))[0] == 1.5
    assert V.diamond(F(-1), F(-1))[0] == 2.5 and V.diamond(F(2), F(-2))[0] == 3.5
    up = float(F(1.001))
    # the ordinary arc [0.5, 1.5]: both bounds are in view (a miss is paid), a hair beyond either is outside (c stays)
    assert one(1, 1, 0.5, 1.5) == (4, 0) and one(-2, 2, 0.5, 1.5) == (4, 0) and one(0, 1, 0.5, 1.5) == (4, 0)
    assert one(up, 1, 0.5, 1.5) == (5, 1) and one(-2 * up, 2, 0.5, 1.5) == (5, 1) and one(1, -1, 0.5, 1.5) == (5, 1)
    # the wrapping arc [2.5, 1.5]: blind between 1.5 and 2.5
    assert one(-1, -1, 2.5, 1.5) == (4, 0) and one(-2, 2, 2.5, 1.5) == (4, 0) and one(1, 0, 2.5, 1.5) == (4, 0)
    assert one(-1, 0, 2.5, 1.5) == (5, 1) and one(-2 * up, 2, 2.5, 1.5) == (5, 1) and one(-up, -1, 2.5, 1.5) == (5, 1)
    assert one(1, -1e-45, 2.5, 1.5) == (4, 0)                     # p = 4
    # lo == hi: one direction; the landmark at the sensor has no direction and is in view
    assert one(1, 1, 0.5, 0.5) == (4, 0) and one(1, 2, 0.5, 0.5) == (5, 1) and one(0, 0, 0.5, 0.5) == (4, 0)
    # outside with nothing to pay: not pruned; a hit counts whatever the direction
    assert one(-1, 0, 2.5, 1.5, c=0) == (0, 1) and one(-1, 0, 2.5, 1.5, c=3, tab=0) == (5, 0)


def test_nan_is_never_outside(orc):
    nan = float("nan")
    for zx, zy in ((nan, 1.0), (1.0, nan), (nan, nan)):
        assert one(zx, zy, 0.5, 0.5) == (5, 0)                    # a NaN mean is not visible: not due, so neither a miss nor outside
    mp = np.zeros((1, 5, 1), F)
    mp[0, 0, 0], mp[0, 2, 0] = -1.0, 0.3
    z = np.zeros(1, F)
    for bad in (nan, float("inf")):                               # a heading without a direction: the landmark has no bin and is in view
        _, ev, _, _, out = V.evidence(mp, z, z, np.array([bad], F), None, np.array([[255]], np.uint8), 1, np.array([[5]], np.uint8), HIT,
                                      MISS, CMAX, RANGE, F(0.5), F(0.5))
        assert (int(ev[0, 0]), int(out[0])) == (4, 0)
    with pytest.raises(AssertionError):
        one(1, 1, nan, 1.0)


@pytest.mark.parametrize("bounds", [(0.5, 1.5), (2.6, 1.4), (0.0, 4.0)])
@pytest.mark.parametrize("sight", [False, True])
def test_every_due_landmark_is_accounted_for_once(orc, bounds, sight):
    mp, x, y, th, tab, ev, anc, T, L = random_case(11, n=40, L=30)
    K = 2
    got = V.evidence(mp, x, y, th, anc, tab, K, ev, HIT, MISS, CMAX, RANGE, F(bounds[0]), F(bounds[1]), *((T, 0.3) if sight else ()), L=L)
    _, ev_out, stats, spared, outside = got
    c = ev[anc][:, :L].astype(int)
    seen = ~(mp[:, 2, :L] < 0)
    dx, dy = mp[:, 0, :L] - x[:, None], mp[:, 1, :L] - y[:, None]
    with np.errstate(all="ignore"):
        due = seen & ~(tab[:, :L] < K) & (dx * dx + dy * dy <= F(RANGE) * F(RANGE))
    pruned = stats[:, 0]
    kept = seen & (got[0][:, 2, :L] >= 0)
    paid = (due & kept & (ev_out[:, :L].astype(int) == c - MISS)).sum(axis=1)
    assert np.array_equal(outside + spared + paid + pruned, due.sum(axis=1))
    assert due.sum() > 50 and pruned.sum() > 0 and paid.sum() > 0
    assert (outside.sum() > 0) == (bounds != (0.0, 4.0)) and (spared.sum() > 0) == sight


def test_fov_bound_is_the_spec_on_the_c_librarys_cosine_and_sine():
    pkg = load_package()
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in (libm.cosf, libm.sinf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    extra = [0.0, -0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2, np.pi / 4, 3.0, -3.0, 1e-30, 100.0]
    angles = np.concatenate([ANGLES, extra]).astype(F)
    got = np.array([pkg.fov_bound(a) for a in angles], F)
    co, si = (np.array([f(float(a)) for a in angles], F) for f in (libm.cosf, libm.sinf))
    want, has = V.diamond(co, si)
    assert has.all() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all((got >= 0) & (got <= 4))
    # strictly increasing over the sensor's 1079 angles once the wrap at p = 4 = 0 is accounted for (the scan starts in the third
    # quadrant, p > 2, passes p = 4 = 0 at angle 0 and ends in the second, p < 2)
    p = got[:1079].astype(np.float64)
    assert np.all(np.diff(np.where(ANGLES < 0, p - 4.0, p)) > 0)
    assert 2.0 < p[0] < 3.0 and 1.0 < p[-1] < 2.0
    assert pkg.fov_bound(float("nan")) == 0.0 and pkg.fov_bound(float("inf")) == 0.0
    # and against the float64 bounds the CPU behaviour test builds: the same direction to within float32 rounding of cos and sin
    assert np.max(np.abs(got[:1079] - V.bound(angles[:1079].astype(np.float64)))) < 1e-6


def test_host_program_refuses_a_bad_edge(tmp_path):
    """slam_pf_main --prune-fov: EDGE is checked while the arguments are read, before any engine call."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    base = [str(exe), str(tmp_path / "none.csv"), "4", "1079", str(tmp_path / "map.csv"), "256", "3", "--landmarks", "32", "--assoc", "9.21", "50"]
    prune = ["--prune", "1", "1", "3", "10"]
    for bad in ("-0.1", "nan", "inf", "abc", "0.1x"):
        r = subprocess.run(base + prune + ["--prune-fov", bad, "--detect"], capture_output=True, text=True)
        assert r.returncode == 2 and "--prune-fov" in r.stderr and "EDGE" in r.stderr, (bad, r.stderr)
    r = subprocess.run(base + ["--prune-fov", "0.1", "--detect"], capture_output=True, text=True)   # without --prune: the usage
    assert r.returncode == 2 and "--prune-fov EDGE" in r.stderr
