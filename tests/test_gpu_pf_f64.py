"""The particle-filter kernels against the independent float64 reference (tests/_f64_pf.py) DIRECTLY — not through the
CPU specification — within the forward-error bounds of tests/test_pf_f64_spec.py (written out in _f64_pf.update_errors,
motion_errors and resample_check).

The parity tests pin every kernel bit for bit to oracle/slam_oracle_pf.c, which restates the kernels' own algebra; what
is checked here is that the numbers are right: the motion sample in every slot, the landmark update and log-likelihood
of every out-of-place and in-place form, and whole session frames (motion, score, update, weights, resample) on the rows,
split, pages and split-pages layouts with frame fusion on and off — over priors from 1e-4 q to 1e8 q with condition
numbers up to 1e4, ~1e10 m^2 priors in the same wavefronts as ordinary ones (the division fallback of the device
reciprocal), poses and landmarks up to 1e3 m away, headings up to 1e3 rad, first sightings, observation lists that are
empty, single, complete and out of order.
"""
import numpy as np
import pytest
import torch

import _f64_pf as F
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    torch.cuda.synchronize()
    e.close()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 65536])
def test_motion_sample_every_slot(eng, n):
    rng = np.random.default_rng(n)
    m = n + 5
    src = [rng.uniform(-1e3, 1e3, m).astype(np.float32) for _ in range(3)]
    anc = np.sort(rng.integers(0, m, n)).astype(np.int32)
    dp, sig = [0.004, -0.001, 0.0006], [0.05, 3.0, 0.01]
    out = [torch.empty(n, device=DEV) for _ in range(3)]
    eng.motion_sample_dev([dev(a) for a in src], dev(anc), out, n, 1 << 32, dp, sig, 0xABCDEF0123, 9)
    r = F.motion_errors([host(t) for t in out], src, anc, dp, sig, 1 << 32, 0xABCDEF0123, 9)
    print(f"motion n={n}: max error / bound {r.max():.3g}")
    assert r.max() <= 1.0


def _obs(rng, L, kind):
    """observation ids of one frame: none, one, every landmark (shuffled) or a shuffled subset"""
    if kind == "none":
        return np.zeros(0, np.int64)
    if kind == "one":
        return rng.integers(0, L, 1)
    ids = rng.permutation(L)
    return ids if kind == "all" else ids[: max(1, L * 2 // 3)]


# (n, L, Lp): landmark counts around the 128-landmark batches and the 64-lane halves, rows tight and padded
EKF_SHAPES = [(1, 1, 1), (63, 31, 32), (64, 32, 32), (65, 33, 40), (63, 127, 128), (64, 128, 128), (65, 129, 160),
              (4097, 255, 256), (64, 256, 256), (65, 257, 257), (63, 500, 512), (4097, 513, 513)]


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("q", [1e-8, 1e-4, 1e-2])
def test_ekf_update_out_of_place(eng, form, q):
    """slam_ekf_update_dev, each out-of-place form, with a fused ancestor gather."""
    eng.ekf_form_set(form)
    try:
        for i, (n, L, Lp) in enumerate(EKF_SHAPES):
            rng = np.random.default_rng(1000 * i + form)
            rows_n = n + 3
            pose, mp, zx, zy = F.mixed_frame(rng, rows_n, L, q)
            pad = np.full((rows_n, 5, Lp), -555.0, np.float32)
            pad[:, :, :L] = mp
            anc = np.sort(rng.integers(0, rows_n, n)).astype(np.int32)
            x, y, th = (p[anc] for p in pose)   # each slot observes from its ancestor's pose
            ids = _obs(rng, L, ["all", "subset", "one", "none", "subset", "all"][i % 6])
            d_out = torch.full((rows_n, 5, Lp), -777.0, device=DEV)
            ll = torch.empty(n, device=DEV)
            eng.obs_upload(ids.astype(np.int32), zx[ids], zy[ids], L)
            eng.ekf_update_dev(dev(pad), d_out, 5 * Lp, Lp, L, dev(x), dev(y), dev(th), dev(anc), n, q, ll)
            got = host(d_out)
            assert np.all(got[n:] == -777.0)
            F.check_frame(pad[anc], got[:n], host(ll), (x, y, th), ids, zx[ids], zy[ids], q,
                          f"form {form} q={q:g} n={n} L={L} Lp={Lp} obs={len(ids)}", L=L)
    finally:
        eng.ekf_form_set(-1)


@pytest.mark.parametrize("form", [0, 1])
def test_ekf_update_in_place(eng, form):
    """The in-place forms (whole rows; the compact list of observed landmarks), observations from a host list and from a
    device table."""
    eng.ekf_inplace_form_set(form)
    try:
        for i, (n, L, Lp) in enumerate(EKF_SHAPES):
            q = [1e-8, 1e-4, 1e-2][i % 3]
            rng = np.random.default_rng(7000 + 10 * i + form)
            pose, mp, zx, zy = F.mixed_frame(rng, n, L, q)
            pad = np.full((n, 5, Lp), -555.0, np.float32)
            pad[:, :, :L] = mp
            ids = _obs(rng, L, ["subset", "all", "none", "one", "all", "subset"][i % 6])
            if i % 2:
                eng.obs_upload(ids.astype(np.int32), zx[ids], zy[ids], L)
            else:
                tx, ty = np.full(L, np.nan, np.float32), np.full(L, np.nan, np.float32)
                tx[ids], ty[ids] = zx[ids], zy[ids]
                tabs = (dev(tx), dev(ty))
                eng.obs_set_dev(tabs[0], tabs[1], L)
            d = dev(pad)
            ll = torch.empty(n, device=DEV)
            eng.ekf_update_dev(d, d, 5 * Lp, Lp, L, *(dev(p) for p in pose), None, n, q, ll)
            got = host(d)
            assert np.array_equal(got[:, :, L:], pad[:, :, L:])
            F.check_frame(pad, got, host(ll), pose, ids, zx[ids], zy[ids], q,
                          f"in place form {form} q={q:g} n={n} L={L} Lp={Lp} obs={len(ids)}", L=L)
    finally:
        eng.ekf_inplace_form_set(-1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 65536])
def test_weights_and_ancestors(eng, n):
    """log-weights, quantised weights and the resample's ancestors (one launch each, as the staged form runs them)."""
    rng = np.random.default_rng(n + 11)
    ll = (rng.standard_normal(n) * 30 - 500).astype(np.float32)
    score = rng.uniform(0, 200, n).astype(np.float32)
    gain = 0.25
    d_lw, d_max = torch.empty(n, device=DEV), torch.empty(1, device=DEV)
    eng.logweight_dev(dev(score), dev(ll), gain, n, d_lw, d_max)
    lw = host(d_lw)
    b = 2 * F.U * (np.abs(ll) + np.abs(np.float32(gain) * score.astype(np.float64)))
    assert (np.abs(lw - F.logweights(ll, score, gain)) <= b).all() and host(d_max)[0] == lw.max()
    d_wq, d_sum = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV)
    eng.quantise_weights_dev(d_lw, d_max, n, d_wq, d_sum)
    wq = host(d_wq).view(np.uint64)
    _, w64 = F.weights(lw)
    e = w64 * (6 * F.U + 2 * F.U * np.abs(lw.astype(np.float64) - float(lw.max()))) + 1.0
    assert (np.abs(wq.astype(np.float64) - w64) <= e).all() and int(host(d_sum).view(np.uint64)[0]) == int(wq.sum())
    for frame in (0, 5):
        d_anc = torch.empty(n, dtype=torch.int32, device=DEV)
        eng.logweight_dev(dev(score), dev(ll), gain, n, d_lw, d_max)   # leaves the block maxima the scan needs
        eng.quantise_scan_dev(d_lw, None, n, None)
        eng.ancestors_from_scan_dev(n, 99, frame, d_anc)
        nd, dc = F.resample_check(wq, host(d_anc), lw, 99, frame)
        print(f"n={n} frame {frame}: {nd} slots off the float64 resample, count difference {dc}")


# ---------------------------------------------------------------- whole session frames

def _world(eng, rng):
    rows, cols, ld = 150, 190, 200
    occ = np.zeros((ld, ld), np.int32)
    occ[:rows, :cols] = rng.random((rows, cols)) < 0.02
    eng.grid_upload(0, occ, load_package().grid_meta(rows, cols, ld, 0.1, -3.0, -2.5), 10.0, want_edt=True)
    ang = np.linspace(-np.pi, np.pi, 360, endpoint=False)
    rad = rng.uniform(1.0, 6.0, 360)
    eng.scan_upload((rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32))


def _families(rng, n):
    """runs of 1 .. 64 neighbouring particles; the index of each particle's run head"""
    fam = np.zeros(n, np.int64)
    i = 0
    while i < n:
        k = int(rng.integers(1, 65))
        fam[i:i + k] = i
        i += k
    return fam


def _session_frames(layout, n, L, q, fusion, frames=4, sample=4096):
    """Frames of a PfSession (every frame resamples).  Before each step: the pending ancestors, the source poses and the
    rows of every current particle (slam_pf_get_map_rows_host applies the pending gather, so these are the ancestors' rows).
    After it: every slot's pose, and for a sample of slots s (all of them up to 4 097) the row and log-likelihood of the
    particle that slot s now descends from, a = anc'[s]; the log-weights and the new ancestors of every slot."""
    pkg = load_package()
    rng = np.random.default_rng(n + L + int(fusion))
    eng = pkg.Engine(0)
    eng.frame_fusion_set(fusion)
    _world(eng, rng)
    sigma, gain, seed = (0.05, 0.05, 0.01), 0.02, 4242
    ses = pkg.PfSession(eng, n, L, sigma=sigma, meas_var=q, score_gain=gain, seed=seed, map_layout=layout)
    try:
        assert ses.layout() == layout
        pose, mp, zx, zy = F.mixed_frame(rng, n, L, q, first_frac=0.05)
        if layout.startswith("split"):   # covariance classes: families of 1 .. 64 particles share their head's covariances
            mp[:, 2:5] = mp[_families(rng, n), 2:5]
        ses.set_poses(*pose)
        ses.set_map(mp)
        eng.sync()
        for f in range(frames):
            v = ses.device_view()
            anc = None if v["anc"] is None else torch.as_tensor(v["anc"], device=DEV).cpu().numpy()
            src = torch.as_tensor(v["pose"], device=DEV).cpu().numpy()
            prior = ses.map_rows(np.arange(n, dtype=np.int32))            # [n][5][L], the ancestors' rows
            ids = _obs(rng, L, ["all", "none", "one", "subset"][f % 4])
            eng.obs_upload(ids.astype(np.int32), zx[ids], zy[ids], L)
            ses.step(0, [0.01, -0.02, 0.003], True)
            eng.sync()
            v = ses.device_view()
            t = lambda k: torch.as_tensor(v[k], device=DEV).cpu().numpy()
            new_pose, ll, lw, score, anc_new = t("pose"), t("loglik"), t("logw"), t("score"), t("anc")
            r = F.motion_errors(new_pose, src, anc, [0.01, -0.02, 0.003], sigma, 0, seed, f)
            assert r.max() <= 1.0, f"frame {f}: motion error {r.max():.3g} x its bound"
            s = np.arange(n) if n <= sample else np.unique(np.concatenate(
                [rng.integers(0, n, sample), [0, 1, n // 2, n - 2, n - 1]]))
            a = anc_new[s]
            got = ses.map_rows(s.astype(np.int32))
            F.check_frame(prior[a], got, ll[a], tuple(p[a] for p in new_pose), ids, zx[ids], zy[ids], q,
                          f"{layout} fusion={fusion} n={n} L={L} frame {f} obs={len(ids)}")
            b = 2 * F.U * (np.abs(ll) + np.abs(np.float32(gain) * score.astype(np.float64)))
            assert (np.abs(lw - F.logweights(ll, score, gain)) <= b).all(), f"frame {f}: log-weights"
            nd, dc = F.resample_check(None, anc_new, lw, seed, f)
            print(f"  frame {f}: {nd} slots off the float64 resample, count difference {dc}")
    finally:
        ses.close()
        eng.close()
        torch.cuda.empty_cache()


LAYOUTS = ["rows", "split", "pages", "split_pages"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,L,q", [(63, 31, 1e-2), (65, 129, 1e-4), (4097, 257, 1e-8), (64, 513, 1e-2)])
def test_session_frames(layout, n, L, q):
    _session_frames(layout, n, L, q, fusion=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fusion", [True, False])
def test_session_frames_64k_x_500(layout, fusion):
    """65 536 x 500, the headline shape: the fused frame front where the layout has one, the two launches otherwise."""
    _session_frames(layout, 65536, 500, 1e-2, fusion=fusion, frames=3)


def test_split_session_frames_more_shapes():
    """Split-layout shapes outside the lists above: a population that is not a multiple of any group size, two launches;
    65 536 x 200, the fused front launch."""
    _session_frames("split", 4097, 257, 1e-2, fusion=False, frames=2)
    _session_frames("split", 65536, 200, 1e-2, fusion=True, frames=2)
