"""A rows session with data association under a covariance per detection (slam_pf_assoc_detcov_set, the covariances uploaded
behind every hand-over of detections) against the frame loop of tests/_assoc_detcov_spec.py, frame by frame and bit for bit:
poses, map rows, log-weights, ancestors, the view's table and stats and the evidence — ungated, gated (kept and resampled
frames), refining and pruning; every Q_k equal against a slam_pf_assoc_cov_set session; the ways back; the frame without
covariances, which launches nothing; the refusals."""
import numpy as np
import pytest
import torch

import subprocess

import _assoc_aniso_spec as AA
import _assoc_detcov_spec as AD
import _detect_noise_spec as DN
import _detect_spec as D
import oracle
import _assoc_spec as A
import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import bits
from test_gpu_assoc_aniso_session import COV, GATE_ESS, KW_SPEC, PRUNE, counters as parent_counters, run_session as run_parent
from test_gpu_assoc_session import DP, FRAMES, GATE, KW, L, N, NEW_GATE, REFINE, _engine, compare, detections, world   # noqa: F401 - world is a fixture

from test_gpu_detect_session import SCANS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANGE_VAR, BEARING_VAR, LATERAL_VAR = 0.01, 0.002, 0.005


def covs_of(zx, zy):
    """Q_k = a u u^T + b v v^T of each detection: a = RANGE_VAR along its line of sight, b = BEARING_VAR r^2 + LATERAL_VAR across."""
    zx, zy = zx.astype(np.float64), zy.astype(np.float64)
    r2 = zx * zx + zy * zy
    ux, uy = zx / np.sqrt(r2), zy / np.sqrt(r2)
    a, b = RANGE_VAR, BEARING_VAR * r2 + LATERAL_VAR
    q = tuple(v.astype(np.float32) for v in (a * ux * ux + b * uy * uy, (a - b) * ux * uy, a * uy * uy + b * ux * ux))
    assert AD.valid_covs(q)
    return q


def feed(world, f):
    zx, zy = detections(world, f)
    return zx, zy, covs_of(zx, zy)


def reference(world, frames=FRAMES, det=None, **kw):
    return AD.frame_loop(world, N, frames, dp=DP, detections=det or (lambda f: feed(world, f)), gate=GATE, new_gate=NEW_GATE, create=1,
                         **kw, **KW_SPEC)


def counters(e):
    return dict(parent_counters(e), detcov=e.assoc_detcov_counts())


def on(pkg, ses):
    ses.assoc_detcov_set(GATE, NEW_GATE, True)


def run_session(world, switch=on, ess=0.0, refine=None, frames=FRAMES, prune=None, layout="rows", comm_group=None, det=None, first=None,
                scans=None):
    """One session over `frames` frames; switch(pkg, ses) in front of frame 0; det(f) -> (zx, zy, covs or None) handed over in front
    of frame f; first(pkg, e, ses): called in front of frame 0's hand-over (the frame that is refused); scans: another scan every
    frame and NO hand-over (the session's detector makes the detections).
    -> per frame what the reference returns, and the counters' advance."""
    pkg = load_package()
    e = _engine(world)
    comm = pkg.Comm.local(e, comm_group, 0) if comm_group else None
    ses = pkg.PfSession(e, N, L, comm=comm, resample_ess_frac=ess, map_layout=layout, **KW)
    if refine:
        ses.refine_set(*refine)
    switch(pkg, ses)
    ses.set_poses(world["x"], world["y"], world["th"])
    ses.set_map(world["mp"])
    if prune:
        ses.prune_set(*prune)
    e.sync()
    c0 = counters(e)
    extra = first(pkg, e, ses) if first else None
    out = []
    for f in range(frames):
        e.obs_upload(*W.observations(world["lm"], f), L)      # (ignored while association is on)
        if scans:
            e.scan_upload(*scans[f])
        else:
            zx, zy, covs = (det or (lambda g: feed(world, g)))(f)
            e.detections_upload(zx, zy)
            if covs is not None:
                e.detections_cov_upload(*covs)
        ses.step(0, DP, True)
        v = ses.device_view()
        e.sync()
        fr = dict(pose=ses.poses(), map=ses.maps(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
                  anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy() if v["anc"] is not None else None)
        if scans:
            fr["det"] = e.detections() + (e.detections_cov(),)
        try:
            av = ses.assoc_view()
            fr["assoc"] = torch.as_tensor(av["assoc"], device=DEV).cpu().numpy()
            fr["stats"] = torch.as_tensor(av["stats"], device=DEV).cpu().numpy()
        except pkg.SlamError:
            pass
        if prune:
            fr["ev"] = ses.evidence()
            fr["ev_stats"] = torch.as_tensor(ses.evidence_view()["stats"], device=DEV).cpu().numpy()
        out.append(fr)
    c1 = counters(e)
    res = dict(frames=out, resampled=ses.frames_resampled(), extra=extra,
               **{k: tuple(np.subtract(c1[k], c0[k]).tolist()) if isinstance(c1[k], tuple) else c1[k] - c0[k] for k in c1})
    ses.close()
    if comm:
        comm.close()
    e.close()
    return res


def only_the_new_stages(got, frames=FRAMES):
    assert got["detcov"] == (frames, frames) and got["new"] == (0, 0) and got["assoc"] == (0, 0) and got["aniso"] == 0, got
    assert got["fused"] == 0 and got["forms"] == (0, 0) and got["inplace"] == (0, 0), got


def test_ungated_session_equals_the_spec(world):
    want = reference(world)
    st = np.stack([w["stats"] for w in want])
    assert st[..., 0].sum() > 0 and st[..., 1].sum() > 0
    one_q = AA.frame_loop(world, N, 1, dp=DP, detections=lambda f: detections(world, f), meas_cov=COV, gate=GATE, new_gate=NEW_GATE, create=1,
                          **KW_SPEC)
    assert not np.array_equal(bits(one_q[0]["map"]), bits(want[0]["map"]))            # (not a single-Q session's maps)
    got = run_session(world)
    compare(got["frames"], want, "ungated")
    only_the_new_stages(got)


def test_gated_session_equals_the_spec(world):
    """The resample gate: the spec alone (checked here, on the CPU) keeps some frames and resamples others; the frame behind a
    kept one associates and updates in place."""
    want = reference(world, ess=GATE_ESS)
    verdicts = [w["resampled"] for w in want]
    assert True in verdicts[:-1] and False in verdicts[:-1], verdicts
    got = run_session(world, ess=GATE_ESS)
    compare(got["frames"], want, "gated")
    assert got["resampled"] == sum(verdicts[:-1])   # the host has looked at every frame but the last
    only_the_new_stages(got)


def test_refining_session_equals_the_spec(world):
    want = reference(world, refine=REFINE)
    got = run_session(world, refine=REFINE)
    compare(got["frames"], want, "refining")
    only_the_new_stages(got)


def test_pruning_session_equals_the_spec(world):
    want = reference(world, prune=PRUNE, ess=GATE_ESS)
    got = run_session(world, prune=PRUNE, ess=GATE_ESS)
    compare(got["frames"], want, "pruning")
    for f, (g, w) in enumerate(zip(got["frames"], want)):
        assert np.array_equal(g["ev"], w["ev"]), f"frame {f}: evidence"
        assert np.array_equal(g["ev_stats"], w["ev_stats"]), f"frame {f}: evidence stats"
    only_the_new_stages(got)
    assert got["evidence"][0] == FRAMES


def test_every_covariance_equal_is_an_assoc_cov_set_session(world):
    same = lambda f: detections(world, f) + (tuple(np.full(len(detections(world, f)[0]), v, np.float32) for v in COV),)
    a = run_session(world, det=same)
    b = run_parent(world, lambda pkg, ses: ses.assoc_cov_set(COV, GATE, NEW_GATE, True))
    compare(a["frames"], [dict(fr, assoc=fr["assoc"][:, :L]) for fr in b["frames"]], "all Q_k equal against assoc_cov_set")
    only_the_new_stages(a)
    assert b["new"] == (FRAMES, FRAMES)


def test_the_ways_back(world):
    """slam_pf_assoc_set(gate), slam_pf_assoc_cov_set and slam_pf_assoc_set(0) behind the switch run exactly what a session that
    never made the call runs."""
    def to_isotropic(pkg, ses):
        on(pkg, ses)
        ses.assoc_set(GATE, NEW_GATE, True)

    want = A.frame_loop(world, N, 2, dp=DP, detections=lambda f: detections(world, f), gate=GATE, new_gate=NEW_GATE, create=1, **KW)
    got = run_session(world, to_isotropic, frames=2)
    compare(got["frames"], want, "assoc_set behind assoc_detcov_set")
    assert got["assoc"] == (2, 2) and got["detcov"] == (0, 0) and got["new"] == (0, 0) and got["fused"] == 0

    def to_one_q(pkg, ses):
        on(pkg, ses)
        ses.assoc_cov_set(COV, GATE, NEW_GATE, True)

    want = AA.frame_loop(world, N, 2, dp=DP, detections=lambda f: detections(world, f), meas_cov=COV, gate=GATE, new_gate=NEW_GATE, create=1,
                         **KW_SPEC)
    got = run_session(world, to_one_q, frames=2)
    compare(got["frames"], want, "assoc_cov_set behind assoc_detcov_set")
    assert got["new"] == (2, 2) and got["detcov"] == (0, 0) and got["assoc"] == (0, 0)

    def off(pkg, ses):
        on(pkg, ses)
        ses.assoc_set(0.0, 0.0, False)

    plain = run_session(world, lambda pkg, ses: None, frames=2)
    back = run_session(world, off, frames=2)
    compare(back["frames"], plain["frames"], "switched off", table=False)
    assert back["detcov"] == (0, 0) and back["assoc"] == (0, 0)
    assert back["fused"] == plain["fused"] and back["forms"] == plain["forms"] and back["inplace"] == plain["inplace"]


def test_a_frame_without_covariances_launches_nothing(world):
    """Detections without covariances, and with the session's detector on without a noise model (it installs detections
    without): SLAM_ERR_NOT_READY before the first launch — no counter moves, frame_fusion_count included — and the frames behind it equal the spec's."""
    def bad_frames(pkg, e, ses):
        c0 = counters(e)
        e.detections_upload(*detections(world, 0))
        for _ in range(2):
            with pytest.raises(pkg.SlamError) as err:
                ses.step(0, DP, True)
            assert err.value.status == -4 and "carry none" in str(err.value), str(err.value)
        e.detections_cov_upload(*covs_of(*detections(world, 0)))
        ses.detect_set()
        with pytest.raises(pkg.SlamError) as err:
            ses.step(0, DP, True)
        assert err.value.status == -4
        ses.detect_set(None)                                             # the detector off again
        e.sync()
        assert counters(e) == c0

    got = run_session(world, first=bad_frames, frames=2)
    compare(got["frames"], reference(world, frames=2), "behind the refused frames")
    only_the_new_stages(got, 2)


def _refused(text):
    def switch(pkg, ses):
        with pytest.raises(pkg.SlamError) as err:
            ses.assoc_detcov_set(GATE, NEW_GATE, True)
        assert err.value.status == -2 and text in str(err.value), str(err.value)
    return switch


def _plain(pkg, ses):
    pass


@pytest.mark.parametrize("layout", ["split", "pages", "auto"])
def test_refused_off_the_row_layout(world, layout):
    plain = run_session(world, _plain, layout=layout, frames=2)
    asked = run_session(world, _refused("row layout"), layout=layout, frames=2)
    compare(asked["frames"], plain["frames"], layout, table=False)
    assert asked["detcov"] == (0, 0) and asked["assoc"] == (0, 0) and asked["fused"] == plain["fused"]


def test_refused_when_sharded_and_under_a_standing_covariance(world):
    pkg = load_package()
    group = pkg.LocalGroup(1)
    plain = run_session(world, _plain, frames=2)
    asked = run_session(world, _refused("not sharded"), frames=2, comm_group=group)
    group.close()
    compare(asked["frames"], plain["frames"], "sharded", table=False)
    assert asked["detcov"] == (0, 0)

    def standing(pkg, ses):
        ses.meas_cov_set(COV)
        _refused("2x2 measurement covariance")(pkg, ses)
        for bad in ((0.0, 50.0), (-1.0, 50.0), (float("nan"), 50.0), (9.21, 1.0)):
            with pytest.raises(pkg.SlamError) as err:
                ses.assoc_detcov_set(*bad, True)
            assert err.value.status == -2

    def only_standing(pkg, ses):
        ses.meas_cov_set(COV)

    a = run_session(world, standing, frames=2)
    b = run_session(world, only_standing, frames=2)
    compare(a["frames"], b["frames"], "under slam_pf_meas_cov_set", table=False)
    assert a["detcov"] == (0, 0) and a["aniso"] == b["aniso"] == 2


NOISE = (1e-4, 1.5625e-4, 1e-4)


def test_the_detectors_noise_model_on_ray_cast_scans(world):
    """slam_pf_detect_noise_set: the detections and their covariances come from each frame's ray-cast scan on the device; they are
    the detector's specification's, and the frames are the spec's stages on them."""
    def detecting(pkg, ses):
        on(pkg, ses)
        ses.detect_noise_set(NOISE)

    a = run_session(world, detecting, scans=SCANS)
    assert a["detect"] == FRAMES
    only_the_new_stages(a)
    x, y, th, mp = (np.ascontiguousarray(world[k][:N]) for k in ("x", "y", "th", "mp"))
    anc = None
    for f in range(FRAMES):
        wx, wy, wq, k, _ = DN.detect_noise(*SCANS[f], None, NOISE)
        zx, zy, q = a["frames"][f]["det"]
        assert k >= 3 and np.array_equal(bits(zx), bits(wx[:k])) and np.array_equal(bits(zy), bits(wy[:k])), f"frame {f}: detections"
        assert all(np.array_equal(bits(g), bits(w[:k])) for g, w in zip(q, wq)), f"frame {f}: covariances"
        x, y, th = oracle.motion_sample(x, y, th, anc, N, 0, DP, KW["sigma"], KW["seed"], f)
        sc, _ = oracle.score_poses_det(world["meta"], world["edt"], *SCANS[f], x, y, th)
        assoc, stats = AD.associate(mp, x, y, th, anc, zx, zy, q, GATE, NEW_GATE, 1)
        mp, ll = AD.update(mp, x, y, th, anc, assoc, zx, zy, q)
        logw, m = oracle.logweight_carry(sc, ll, KW["score_gain"], None)
        wq16, _ = oracle.quantise_weights(logw, m)
        anc = oracle.resample(wq16, KW["seed"], f)
        g = a["frames"][f]
        assert np.array_equal(g["assoc"][:, :L], assoc) and np.array_equal(g["stats"], stats), f"frame {f}: table"
        assert np.array_equal(bits(g["logw"]), bits(logw)) and np.array_equal(g["anc"], anc), f"frame {f}: weights"
        assert np.array_equal(bits(g["map"]), bits(mp[anc])), f"frame {f}: map rows"

    # the two older modes accept the detector with a model and ignore the covariances
    def older(pkg, ses):
        ses.assoc_cov_set(COV, GATE, NEW_GATE, True)
        ses.detect_noise_set(NOISE)

    def older_plain(pkg, ses):
        ses.assoc_cov_set(COV, GATE, NEW_GATE, True)
        ses.detect_set()

    b = run_session(world, older, scans=SCANS, frames=2)
    d = run_parent(world, older_plain, scans=SCANS, frames=2)
    compare(b["frames"], [dict(fr, assoc=fr["assoc"][:, :L]) for fr in d["frames"]], "assoc_cov_set with the model")
    assert b["new"] == (2, 2) and b["detcov"] == (0, 0)


def test_host_program_with_range_noise(orc, tmp_path):
    """slam_pf_main --landmarks --assoc --detect --range-noise --landmarks-out on the pole ring of test_gpu_assoc_aniso_session.py:
    twice, the same bytes out, a finite, non-empty landmark file."""
    ring = np.deg2rad(30.0 * np.arange(12) + 3.0)
    poles = np.stack([(3.0 + 0.1 * np.arange(12)) * np.cos(ring), (3.0 + 0.1 * np.arange(12)) * np.sin(ring)], 1)
    rng = D.raycast((0.0, 0.0, 0.0), poles, 0.1, 6.0, angles=-2.351831 + 0.004363 * np.arange(1079))
    ranges = np.hypot(rng[0].astype(np.float64), rng[1].astype(np.float64))
    room = tmp_path / "room.csv"
    room.write_text("".join(",".join(f"{v:.6f}" for v in ranges) + "\n" for _ in range(24)))
    outs = []
    for run in ("a", "b"):
        lm, mp = tmp_path / f"landmarks_{run}.csv", tmp_path / f"map_{run}.csv"
        r = subprocess.run([str(PKG_DIR / "lib" / "slam_pf_main"), str(room), "24", "1079", str(mp), "256", "3", "--landmarks", "32",
                            "--assoc", "9.21", "50", "--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0", "--range-noise", "0.0004", "0.0002",
                            "0.0004", "--landmarks-out", str(lm)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, lm.read_bytes(), mp.read_bytes()))
    assert outs[0] == outs[1]
    found = np.array([[float(v) for v in ln.split(",")] for ln in outs[0][1].decode().splitlines()])
    assert found.ndim == 2 and found.shape[1] == 2 and 1 <= len(found) <= 32 and np.isfinite(found).all()
    r = subprocess.run([str(PKG_DIR / "lib" / "slam_pf_main"), str(room), "24", "1079", str(tmp_path / "m.csv"), "256", "3", "--landmarks", "32",
                        "--assoc", "9.21", "50", "--range-noise", "0.0004", "0.0002"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2                                             # only with --detect
