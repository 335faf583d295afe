"""slam_argmax_dev (csrc/estimate_kernels.hip: argmax_kernel) against a NumPy restatement of its rule — the largest value, the lowest
index on ties, NaN never wins, index 0 and value -inf with nothing but -inf and NaN — index and value bit for bit; and the same
populations through slam_pf_best (best_particle_kernel: the same block arg-max), which tests/test_gpu_estimates.py drives with
such populations at 2049 and 65 537 only.  The sizes: one thread, around a wavefront, around the one workgroup of 1024 threads and
its 1024-stride loop, and a third turn of that loop."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _estimate_spec as E
import _shard_worker as W
from __graft_entry__ import load_package
from conftest import bits as _bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]


def bits(x):
    """the bit pattern of one float32 as an int"""
    return int(_bits(x).ravel()[0])


def argmax_spec(v):
    """-> (index, value) by the rule, without a loop: among the values that are not NaN the maximum, its first position"""
    v = np.ascontiguousarray(v, np.float32)
    m = np.max(np.where(np.isnan(v), -np.inf, v).astype(np.float32))
    if not m > -np.inf:
        return 0, np.float32(-np.inf)
    i = int(np.flatnonzero(v == m)[0])
    return i, v[i]


def populations(n):
    """name -> float32 [n].  A case that needs two places is left out where n does not hold them (two wavefronts: n > 64; two
    turns of the 1024-stride loop: n > 1024)."""
    rng = np.random.default_rng(n)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    base = rng.normal(-5.0, 1.0, n).astype(np.float32)
    cases = {"random": base, "all equal": np.full(n, -2.5, np.float32)}
    for tag, where in (("two wavefronts", [n - 1, n // 2 - 1]), ("the first two wavefronts", [3, 64 + 5]),
                       ("two 1024-strides", [n - 1, n - 1 - 1024]), ("two 1024-strides and a wavefront", [1024 + 7, 7, 900])):
        where = [w for w in where if 0 <= w < n]
        if len(where) < 2 or (max(where) >> 6) == (min(where) >> 6):
            continue
        lw = base.copy()
        lw[where] = 1.5
        cases["maximum repeated in " + tag] = lw
    lw = base.copy(); lw[n // 2] = inf; cases["+inf present"] = lw
    lw = base.copy(); lw[[n - 1, n // 3]] = inf; cases["+inf twice"] = lw
    cases["only -inf"] = np.full(n, -inf, np.float32)
    cases["only NaN"] = np.full(n, nan, np.float32)
    lw = np.full(n, -inf, np.float32); lw[::3] = nan; cases["only -inf and NaN"] = lw
    lw = base.copy(); lw[int(np.argmax(base))] = nan; cases["NaN where the maximum was"] = lw
    lw = base.copy(); lw[0] = nan; lw[n - 1] = 2.0; cases["NaN first, the maximum last"] = lw
    return cases


@pytest.fixture(scope="module")
def rig(orc):
    pkg = load_package()
    world = W.make_world(L=6)
    eng = pkg.Engine(0)
    meta, edt, bx, by, _ = world
    d_edt = torch.from_numpy(edt).to(DEV)
    eng.grid_set_dev(0, d_edt, pkg.grid_meta(meta.rows, meta.cols, meta.ld, meta.pixel, meta.min_x, meta.min_y))
    eng.scan_upload(bx, by)
    yield SimpleNamespace(pkg=pkg, eng=eng, lm=world[4], keep=d_edt)
    eng.close()


def test_the_populations_hold_their_cases():
    """Every size has the cases one value can make; the tie across wavefronts from 65 on, the tie across the 1024-stride from 1025 on."""
    for n in SIZES:
        names = set(populations(n))
        assert {"random", "all equal", "+inf present", "only -inf", "only NaN", "NaN where the maximum was"} <= names, n
        assert ("maximum repeated in two wavefronts" in names) == (n > 64), n
        assert ("maximum repeated in two 1024-strides" in names) == (n > 1024), n
    assert argmax_spec(np.array([np.nan, -np.inf], np.float32)) == (0, np.float32(-np.inf))
    assert argmax_spec(np.array([np.nan, 1.0, 1.0, np.inf, np.inf], np.float32)) == (3, np.float32(np.inf))
    assert argmax_spec(np.array([np.nan, -3.0, 1.0, 1.0, np.nan], np.float32)) == (2, np.float32(1.0))


@pytest.mark.parametrize("n", SIZES)
def test_argmax_dev_against_the_rule(rig, n):
    d_v = torch.empty(n, dtype=torch.float32, device=DEV)
    d_i = torch.empty(1, dtype=torch.int32, device=DEV)
    d_m = torch.empty(1, dtype=torch.float32, device=DEV)
    for tag, v in populations(n).items():
        d_v.copy_(torch.from_numpy(v))
        d_i.fill_(-7)
        d_m.fill_(123.0)
        torch.cuda.synchronize()
        rig.eng.argmax_dev(d_v, n, d_i, d_m)
        rig.eng.sync()
        wi, wv = argmax_spec(v)
        gi, gv = int(d_i.cpu()[0]), d_m.cpu().numpy()[0]
        assert gi == wi and bits(gv) == bits(wv), (tag, n, gi, wi, float(gv), float(wv))


@pytest.mark.parametrize("n", SIZES)
def test_pf_best_on_the_same_populations(rig, n):
    """Log-weights written through the view (as test_gpu_estimates.py does): the session's heaviest particle is the rule's, with
    its pose, and the restatement of tests/_estimate_spec.py agrees with the one above."""
    x, y, th, _ = W.init_state(n, 0, rig.lm[:0])
    ses = rig.pkg.PfSession(rig.eng, n, 0, seed=E.SEED, sigma=E.SIGMA, meas_var=0.02, score_gain=1.0, comm=None,
                            resample_ess_frac=0.0, map_layout="rows")
    try:
        ses.set_poses(x, y, th)
        ses.step(0, list(E.DP))
        rig.eng.sync()
        view = ses.device_view()
        pose = torch.as_tensor(view["pose"], device=DEV).cpu().numpy()
        d_logw = torch.as_tensor(view["logw"], device=DEV)
        for tag, v in populations(n).items():
            d_logw.copy_(torch.from_numpy(v))
            torch.cuda.synchronize()
            wi, wv = argmax_spec(v)
            sp, sv, si = E.best_spec(v, pose[0], pose[1], pose[2])
            assert (si, bits(sv)) == (wi, bits(wv)), (tag, n)
            gp, gv, gi = ses.best()
            assert gi == wi and bits(gv) == bits(wv) and np.array_equal(_bits(gp), _bits(pose[:, wi])), (tag, n, gi, wi, float(gv), float(wv))
    finally:
        ses.close()
