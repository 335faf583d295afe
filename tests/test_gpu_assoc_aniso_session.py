"""A rows session with data association under a 2x2 measurement covariance (slam_pf_assoc_cov_set) against the frame loop of
tests/_assoc_aniso_spec.py, frame by frame and bit for bit: poses, map rows, log-weights, ancestors and the view's table and
stats — ungated, gated (kept and resampled frames), refining, with pruning (evidence bytes against _evidence_spec) and with the
detector; the switch's interface (the isotropic covariance is slam_pf_assoc_set, the refusals, the ways back, no fused front);
and slam_pf_main with --assoc and --meas-cov together."""
import subprocess

import numpy as np
import pytest
import torch

import _assoc_aniso_spec as AA
import _assoc_spec as A
import _detect_spec as D
import _shard_worker as W
import oracle
from __graft_entry__ import PKG_DIR, load_package
from conftest import bits
from test_gpu_assoc_session import DP, FRAMES, GATE, KW, L, N, NEW_GATE, REFINE, _engine, compare, detections, world   # noqa: F401 - world is a fixture
from test_gpu_detect_session import SCANS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COV = (0.02, 0.012, 0.015)
ISO = (KW["meas_var"], 0.0, KW["meas_var"])
GATE_ESS = 0.03   # with this gate the spec resamples some frames and keeps others (asserted below, on the CPU)
PRUNE = (1, 1, 3, 6.0)
KW_SPEC = {k: v for k, v in KW.items() if k != "meas_var"}


def reference(world, frames=FRAMES, det=None, **kw):
    return AA.frame_loop(world, N, frames, dp=DP, detections=det or (lambda f: detections(world, f)), meas_cov=COV, gate=GATE,
                         new_gate=NEW_GATE, create=1, **kw, **KW_SPEC)


def counters(e):
    return dict(fused=e.frame_fusion_count(), assoc=e.assoc_counts(), new=e.assoc_aniso_counts(), aniso=e.ekf_aniso_count(),
                forms=e.ekf_form_counts(), inplace=e.ekf_inplace_form_counts(), evidence=e.evidence_counts(), detect=e.detect_count())


def run_session(world, switch, ess=0.0, refine=None, frames=FRAMES, prune=None, layout="rows", comm_group=None, scans=None, feed=None):
    """One session over `frames` frames; switch(pkg, ses): what is called on the fresh session in front of frame 0.  scans: another
    scan every frame (the detector's input); feed(f) -> the detections uploaded in front of frame f (default: the world's).
    -> per frame what the reference returns (and `det`: the engine's detections), and the counters' advance."""
    pkg = load_package()
    e = _engine(world)
    comm = pkg.Comm.local(e, comm_group, 0) if comm_group else None
    ses = pkg.PfSession(e, N, L, comm=comm, resample_ess_frac=ess, map_layout=layout, **KW)
    if refine:
        ses.refine_set(*refine)
    extra = switch(pkg, ses)
    ses.set_poses(world["x"], world["y"], world["th"])
    ses.set_map(world["mp"])
    if prune:
        ses.prune_set(*prune)
    c0 = counters(e)
    out = []
    for f in range(frames):
        if scans:
            e.scan_upload(*scans[f])
        e.obs_upload(*W.observations(world["lm"], f), L)      # (ignored while association is on)
        e.detections_upload(*(feed(f) if feed else detections(world, f)))
        ses.step(0, DP, True)
        v = ses.device_view()
        e.sync()
        fr = dict(pose=ses.poses(), map=ses.maps(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
                  anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy() if v["anc"] is not None else None, det=e.detections())
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


def on(pkg, ses):
    ses.assoc_cov_set(COV, GATE, NEW_GATE, True)


def only_the_new_stages(got, frames=FRAMES):
    assert got["new"] == (frames, frames) and got["assoc"] == (0, 0) and got["aniso"] == 0, got
    assert got["fused"] == 0 and got["forms"] == (0, 0) and got["inplace"] == (0, 0), got


def test_ungated_session_equals_the_spec(world):
    want = reference(world)
    st = np.stack([w["stats"] for w in want])
    assert st[..., 0].sum() > 0 and st[..., 1].sum() > 0 and st[..., 2].sum() > 0   # matches, new landmarks and dropped detections
    iso = A.frame_loop(world, N, 1, dp=DP, detections=lambda f: detections(world, f), gate=GATE, new_gate=NEW_GATE, create=1, **KW)
    assert not np.array_equal(bits(iso[0]["map"]), bits(want[0]["map"]))              # (not the isotropic session's maps)
    got = run_session(world, on)
    compare(got["frames"], want, "ungated")
    only_the_new_stages(got)


def test_gated_session_equals_the_spec(world):
    """The resample gate: the spec alone (checked here, on the CPU) keeps some frames and resamples others; the frame behind a
    kept one associates and updates in place."""
    want = reference(world, ess=GATE_ESS)
    verdicts = [w["resampled"] for w in want]
    assert True in verdicts[:-1] and False in verdicts[:-1], verdicts
    got = run_session(world, on, ess=GATE_ESS)
    compare(got["frames"], want, "gated")
    assert got["resampled"] == sum(verdicts[:-1])   # the host has looked at every frame but the last
    only_the_new_stages(got)


def test_refining_session_equals_the_spec(world):
    want = reference(world, refine=REFINE)
    got = run_session(world, on, refine=REFINE)
    compare(got["frames"], want, "refining")
    only_the_new_stages(got)


def test_pruning_session_equals_the_spec(world):
    """slam_pf_prune_set accepts the session: evidence bytes and stats against _evidence_spec.evidence behind the new update."""
    want = reference(world, prune=PRUNE, ess=GATE_ESS)
    got = run_session(world, on, prune=PRUNE, ess=GATE_ESS)
    compare(got["frames"], want, "pruning")
    for f, (g, w) in enumerate(zip(got["frames"], want)):
        assert np.array_equal(g["ev"], w["ev"]), f"frame {f}: evidence"
        assert np.array_equal(g["ev_stats"], w["ev_stats"]), f"frame {f}: evidence stats"
    print("pruned per frame:", [int(w["ev_stats"][:, 0].sum()) for w in want])
    only_the_new_stages(got)
    assert got["evidence"][0] == FRAMES


def test_detecting_session_equals_one_fed_by_hand_and_the_spec(world):
    """slam_pf_detect_set accepts the session: the detections come from each frame's scan, and a session without the detector
    that is handed slam_detections_get_host's output gives the same tables and everything else."""
    def detecting(pkg, ses):
        on(pkg, ses)
        ses.detect_set()

    a = run_session(world, detecting, scans=SCANS, frames=FRAMES)
    dets = [fr["det"] for fr in a["frames"]]
    assert min(len(d[0]) for d in dets) >= 3 and a["detect"] == FRAMES
    for f, (zx, zy) in enumerate(dets):                               # ... and they are the detector's specification's
        wx, wy, k, _ = D.detect(*SCANS[f])
        assert np.array_equal(bits(zx), bits(wx[:k])) and np.array_equal(bits(zy), bits(wy[:k]))
    b = run_session(world, on, scans=SCANS, frames=FRAMES, feed=lambda f: dets[f])
    assert b["detect"] == 0
    compare(a["frames"], [dict(fr, assoc=fr["assoc"][:, :L]) for fr in b["frames"]], "detector against hand-over")
    # the spec's loop scores with one scan; here every frame has its own: frame by frame through the loop's own stages
    x, y, th, mp = (np.ascontiguousarray(world[k][:N]) for k in ("x", "y", "th", "mp"))
    anc = None
    for f in range(FRAMES):
        x, y, th = oracle.motion_sample(x, y, th, anc, N, 0, DP, KW["sigma"], KW["seed"], f)
        sc, _ = oracle.score_poses_det(world["meta"], world["edt"], *SCANS[f], x, y, th)
        assoc, stats = AA.associate(mp, x, y, th, anc, *dets[f], COV, GATE, NEW_GATE, 1)
        mp, ll = AA.update(mp, x, y, th, anc, assoc, *dets[f], COV)
        logw, m = oracle.logweight_carry(sc, ll, KW["score_gain"], None)
        wq, _ = oracle.quantise_weights(logw, m)
        anc = oracle.resample(wq, KW["seed"], f)
        g = a["frames"][f]
        assert np.array_equal(g["assoc"][:, :L], assoc) and np.array_equal(g["stats"], stats), f"frame {f}: table"
        assert np.array_equal(bits(g["logw"]), bits(logw)) and np.array_equal(g["anc"], anc), f"frame {f}: weights"
        assert np.array_equal(bits(g["map"]), bits(mp[anc])), f"frame {f}: map rows"
    only_the_new_stages(a)


def test_the_isotropic_covariance_is_assoc_set(world):
    """meas_cov = {meas_var, 0, meas_var}: the isotropic kernels, the bits of slam_pf_assoc_set, its counters."""
    want = A.frame_loop(world, N, 2, dp=DP, detections=lambda f: detections(world, f), gate=GATE, new_gate=NEW_GATE, create=1, **KW)
    got = run_session(world, lambda pkg, ses: ses.assoc_cov_set(ISO, GATE, NEW_GATE, True), frames=2)
    compare(got["frames"], want, "isotropic covariance")
    assert got["assoc"] == (2, 2) and got["new"] == (0, 0) and got["fused"] == 0


def _refused(text, cov=COV, gates=(GATE, NEW_GATE)):
    def switch(pkg, ses):
        with pytest.raises(pkg.SlamError) as err:
            ses.assoc_cov_set(cov, *gates, True)
        assert err.value.status == -2 and text in str(err.value), str(err.value)
    return switch


def _plain(pkg, ses):
    pass


@pytest.mark.parametrize("layout", ["split", "pages", "auto"])
def test_refused_off_the_row_layout(world, layout):
    """... and the session then steps exactly as one that was never asked."""
    plain = run_session(world, _plain, layout=layout, frames=2)
    asked = run_session(world, _refused("row layout"), layout=layout, frames=2)
    compare(asked["frames"], plain["frames"], layout, table=False)
    assert asked["new"] == (0, 0) and asked["assoc"] == (0, 0) and asked["fused"] == plain["fused"]


def test_refused_when_sharded(world):
    pkg = load_package()
    group = pkg.LocalGroup(1)
    plain = run_session(world, _plain, frames=2)
    asked = run_session(world, _refused("not sharded"), frames=2, comm_group=group)
    group.close()
    compare(asked["frames"], plain["frames"], "sharded", table=False)
    assert asked["new"] == (0, 0)


def test_refusals_on_rows_and_the_ways_back(world):
    def switch(pkg, ses):
        ses.meas_cov_set(COV)                                           # a standing 2x2 covariance: one way in, not two matrices
        _refused("2x2 measurement covariance")(pkg, ses)
        ses.meas_cov_set(ISO)
        for bad in ((float("nan"), 0.0, 1.0), (1.0, 1.0, 1.0), (-1.0, 0.0, 1.0)):
            _refused("meas_cov must be finite", cov=bad)(pkg, ses)
        for bad in ((0.0, 50.0), (-1.0, 50.0), (float("nan"), 50.0), (float("inf"), float("inf")), (9.21, 1.0), (9.21, float("nan"))):
            _refused("gate", gates=bad)(pkg, ses)
        with pytest.raises(pkg.SlamError):
            ses.assoc_view()                                            # nothing was switched on, nothing allocated
        on(pkg, ses)
        with pytest.raises(pkg.SlamError) as err:
            ses.meas_cov_set(COV)                                       # stays refused: association is on
        assert err.value.status == -2 and "data association is on" in str(err.value)
        ses.meas_cov_set(ISO)                                           # the isotropic covariance is no change: accepted
        _refused("meas_cov must be finite", cov=(0.0, 0.0, 1.0))(pkg, ses)   # a refused call changes nothing: the switch stays on

    got = run_session(world, switch, frames=2)
    compare(got["frames"], reference(world, frames=2), "after the refusals")
    only_the_new_stages(got, 2)

    def back_to_isotropic(pkg, ses):
        on(pkg, ses)
        ses.assoc_set(GATE, NEW_GATE, True)

    want = A.frame_loop(world, N, 2, dp=DP, detections=lambda f: detections(world, f), gate=GATE, new_gate=NEW_GATE, create=1, **KW)
    got = run_session(world, back_to_isotropic, frames=2)
    compare(got["frames"], want, "assoc_set behind assoc_cov_set")
    assert got["assoc"] == (2, 2) and got["new"] == (0, 0) and got["fused"] == 0

    def off(pkg, ses):
        on(pkg, ses)
        ses.assoc_set(0.0, 0.0, False)

    plain = run_session(world, _plain, frames=2)
    back = run_session(world, off, frames=2)
    compare(back["frames"], plain["frames"], "switched off", table=False)
    assert back["new"] == (0, 0) and back["assoc"] == (0, 0)
    assert back["fused"] == plain["fused"] and back["forms"] == plain["forms"] and back["inplace"] == plain["inplace"]


def test_host_program_with_assoc_and_meas_cov(orc, tmp_path):
    """slam_pf_main --landmarks --assoc --meas-cov --detect --landmarks-out: the combination that used to exit with the two
    switches' refusal runs to the end and writes a finite, non-empty landmark file (the pole ring of test_gpu_detect_session.py,
    24 frames, 256 particles)."""
    ring = np.deg2rad(30.0 * np.arange(12) + 3.0)
    poles = np.stack([(3.0 + 0.1 * np.arange(12)) * np.cos(ring), (3.0 + 0.1 * np.arange(12)) * np.sin(ring)], 1)
    rng = D.raycast((0.0, 0.0, 0.0), poles, 0.1, 6.0, angles=-2.351831 + 0.004363 * np.arange(1079))
    ranges = np.hypot(rng[0].astype(np.float64), rng[1].astype(np.float64))
    room, lm = tmp_path / "room.csv", tmp_path / "landmarks.csv"
    room.write_text("".join(",".join(f"{v:.6f}" for v in ranges) + "\n" for _ in range(24)))
    r = subprocess.run([str(PKG_DIR / "lib" / "slam_pf_main"), str(room), "24", "1079", str(tmp_path / "map.csv"), "256", "3", "--landmarks", "32",
                        "--assoc", "9.21", "50", "--meas-cov", "0.0004", "0", "0.01", "--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0",
                        "--landmarks-out", str(lm)], capture_output=True, text=True, timeout=120)
    print(r.stderr.strip())
    assert r.returncode == 0, r.stderr
    found = np.array([[float(v) for v in ln.split(",")] for ln in lm.read_text().splitlines()])
    assert found.ndim == 2 and found.shape[1] == 2 and 1 <= len(found) <= 32 and np.isfinite(found).all()
