"""slam_pf_known_map_reseed inside a session against the frame loop of tests/_reseed_spec.py — the localise loops of
_localise_spec.py / _localise_detcov_spec.py extended by the spec's reseed behind chosen frames: poses after every frame and after
every reseed bit for bit, log-weights, ancestors and verdicts of every frame, the counts — resampling every frame and ESS-gated, in
both noise forms; slam_pf_best refused from a reseed to the next step; a session that never reseeds against the unextended loops;
the refusals; and slam_pf_main --known-reseed."""
import subprocess

import numpy as np
import pytest
import torch

import _localise_detcov_spec as SD
import _localise_spec as S
import _reseed_spec as R
import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import GOLDEN, bits
from test_gpu_localise_detcov_session import covs_of
from test_gpu_localise_session import compare, frame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES = 1024, 12, 8
GATE, CLUTTER, GATE_ESS = 9.21, -2.5, 0.5
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
DP = [0.01, -0.005, 0.002]
FRACTIONS = {1: 0.25, 2: 1.0 / 16, 4: 1.0, 5: 0.5, 6: 2.0**-10}   # frame -> the fraction reseeded behind it
NOT_READY = -4


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, bx, by, lm = W.make_world(L=L)
    x, y, th, _ = W.init_state(N, 0, np.zeros((0, 2), np.float32))
    M = np.zeros((5, L), np.float32)
    M[0], M[1], M[2], M[4] = lm[:, 0], lm[:, 1], 0.05, 0.05
    M[3] = 0.01
    M[2, ::5] = -1.0                             # slots that hold no landmark
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), bx=bx, by=by, lm=lm, x=x, y=y, th=th, M=M)


def detections(world, f, detcov):
    """The world's landmark observations of frame f in shuffled order, without their ids (and with a covariance each)."""
    _, zx, zy = W.observations(world["lm"], 0)
    zx, zy = zx + np.float32(0.01 * f), zy + np.float32(0.01 * f)
    pick = np.random.default_rng(100 + f).permutation(len(zx))[:10]
    zx, zy = zx[pick].copy(), zy[pick].copy()
    return (zx, zy, covs_of(zx, zy)) if detcov else (zx, zy)


def spec_kw(detcov):
    return {k: v for k, v in KW.items() if not (detcov and k == "meas_var")}


def reference(world, detcov, ess, reseed_after):
    return R.frame_loop(world, N, FRAMES, dp=DP, detections=lambda f: detections(world, f, detcov), known_map=world["M"], gate=GATE,
                        log_clutter=CLUTTER, ess=ess, reseed_after=reseed_after, **spec_kw(detcov))


def open_session(world, ess=0.0, **kw):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    ses = pkg.PfSession(e, N, kw.pop("n_landmarks", 0), resample_ess_frac=ess, **kw, **KW)
    ses.set_poses(world["x"], world["y"], world["th"])
    return pkg, e, ses


def hand_over(e, world, f, detcov):
    det = detections(world, f, detcov)
    e.detections_upload(det[0], det[1])
    if detcov:
        e.detections_cov_upload(*det[2])


@pytest.mark.parametrize("detcov", [False, True], ids=["meas-var", "per-detection"])
@pytest.mark.parametrize("ess", [0.0, GATE_ESS], ids=["every-frame", "gated"])
def test_session_equals_the_spec_loop(world, ess, detcov):
    want = reference(world, detcov, ess, FRACTIONS.get)
    counts = {f: tuple(want[f]["counts"]) for f in FRACTIONS}
    assert counts[4] == (N - counts[4][1], counts[4][1]) and counts[4][1] > 0 and all(c[0] > 0 for f, c in counts.items() if f != 6)
    pkg, e, ses = open_session(world, ess=ess)
    (ses.known_map_detcov_set if detcov else ses.known_map_set)(world["M"], GATE, CLUTTER)
    c0 = e.pose_reseed_count()
    for f in range(FRAMES):
        hand_over(e, world, f, detcov)
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f}")
        best = ses.best()
        if f in FRACTIONS:
            assert ses.known_map_reseed(FRACTIONS[f]) == counts[f], f"frame {f}: counts"
            assert ses.device_view()["anc"] is None
            got = ses.poses()
            assert np.array_equal(bits(got), bits(want[f]["reseeded"])), f"frame {f}: the reseeded population"
            with pytest.raises(pkg.SlamError, match="reseeded") as err:
                ses.best()
            assert err.value.status == NOT_READY
            if f == 2:   # no step in between: the same draws, now without a pending gather — the proposals land where they landed
                again = R.reseed(world["M"], *got, None, *detections(world, f, False), 0, KW["seed"], f + 1, FRACTIONS[f])
                assert ses.known_map_reseed(FRACTIONS[f]) == tuple(again[4]) == counts[f]
                assert np.array_equal(bits(ses.poses()), bits(np.stack(again[:3]))) and np.array_equal(bits(again[0]), bits(got[0]))
            # equal weights, as after set_poses: the plain mean and the spread about it
            m = ses.mean(0.0)
            sp = ses.spread(0.0)
            assert np.array_equal(bits(sp[0]), bits(m)) and np.allclose(m[:2], ses.poses()[:2].astype(np.float64).mean(axis=1), atol=1e-4)
        else:
            assert best[2] == int(np.argmax(want[f]["logw"]))
    assert e.pose_reseed_count() - c0 == len(FRACTIONS) + 1
    if ess:
        verdicts = [w["resampled"] for w in want]
        print("resample verdicts", verdicts)
        assert ses.frames_resampled() == sum(verdicts[:-1])   # the host has looked at every frame but the last
    ses.close()
    e.close()


@pytest.mark.parametrize("detcov", [False, True], ids=["meas-var", "per-detection"])
@pytest.mark.parametrize("ess", [0.0, GATE_ESS], ids=["every-frame", "gated"])
def test_a_session_that_never_reseeds_runs_the_frames_it_ran_before(world, ess, detcov):
    det = lambda f: detections(world, f, detcov)
    common = dict(dp=DP, detections=det, known_map=world["M"], gate=GATE, log_clutter=CLUTTER, ess=ess, **spec_kw(detcov))
    want = (SD if detcov else S).frame_loop(world, N, FRAMES, **common)
    mine = R.frame_loop(world, N, FRAMES, **common)   # the extended loop without a reseed IS the unextended one
    pkg, e, ses = open_session(world, ess=ess)
    (ses.known_map_detcov_set if detcov else ses.known_map_set)(world["M"], GATE, CLUTTER)
    c0 = e.pose_reseed_count()
    for f in range(FRAMES):
        assert all(np.array_equal(bits(mine[f][k]), bits(want[f][k])) for k in ("pose", "logw")) and np.array_equal(mine[f]["anc"], want[f]["anc"])
        hand_over(e, world, f, detcov)
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f}")
        assert ses.best()[2] == int(np.argmax(want[f]["logw"]))
    assert e.pose_reseed_count() == c0
    ses.close()
    e.close()


def test_refusals_leave_the_session_as_it_was(world):
    pkg = load_package()

    def refused(ses, text, status=NOT_READY, fraction=0.5):
        with pytest.raises(pkg.SlamError, match=text) as err:
            ses.known_map_reseed(fraction)
        assert err.value.status == status

    want = reference(world, False, 0.0, None)
    _, e, ses = open_session(world)
    c0 = e.pose_reseed_count()
    hand_over(e, world, 0, False)
    refused(ses, "mode is off")
    ses.known_map_set(world["M"], GATE, CLUTTER)
    for bad in (0.0, -1.0, 1.5, float("nan")):
        refused(ses, "fraction", status=-2, fraction=bad)
    for f in range(2):
        hand_over(e, world, f, False)
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f}")
        e.detections_upload(np.zeros(0, np.float32), np.zeros(0, np.float32))
        assert ses.known_map_reseed(1.0) == (0, 0)      # K == 0: nothing happens, the gather stays pending, best still answers
        assert ses.device_view()["anc"] is not None and ses.best()[2] == int(np.argmax(want[f]["logw"]))
    ses.known_map_set(None)
    refused(ses, "mode is off")
    assert e.pose_reseed_count() == c0
    ses.close()
    e.close()

    _, e, ses = open_session(world, n_landmarks=8, map_layout="rows")
    hand_over(e, world, 0, False)
    refused(ses, "n_landmarks > 0")
    ses.close()
    e.close()

    fresh_pkg, e, ses = open_session(world)   # a known map, and no detections were ever handed over
    ses.known_map_set(world["M"], GATE, CLUTTER)
    refused(ses, "no detections")
    ses.close()
    e.close()


def test_host_program_reseeds(orc, tmp_path):
    """slam_pf_main --known-map --known-reseed on the head of the recorded dataset: every frame's line carries the two counts —
    all of the population or, where the detector found no pole in the frame's scan (K == 0), nothing; only every second frame with
    EVERY = 2; without the switch the lines are what they were; refused without --known-map and with a bad FRACTION or EVERY.  (The
    counts themselves: the session test above.)"""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv = GOLDEN / "frames_head.csv"
    lines = csv.read_text().splitlines()
    base = [str(exe), str(csv), str(len(lines)), str(len(lines[1].split(",")))]
    km = tmp_path / "known.csv"
    km.write_text("".join(f"{x:f},{y:f}\n" for x, y in np.random.default_rng(3).uniform(-8, 8, (20, 2))))
    known = ["--known-map", str(km), "9.21", "0.05", "-2.5", "--detect"]
    r = subprocess.run(base + [str(tmp_path / "m0.csv"), "256", "3"] + known + ["--known-reseed", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tails = [ln.split("reseed = ")[1].split() for ln in r.stdout.splitlines() if ln.startswith("pose =")]
    assert len(tails) == len(lines) - 1 and all(t in (["256", "0"], ["0", "0"]) for t in tails)
    r = subprocess.run(base + [str(tmp_path / "m1.csv"), "256", "3"] + known + ["--known-reseed", "0.5", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tails = [ln.split("reseed = ")[1].split() for ln in r.stdout.splitlines() if ln.startswith("pose =")]
    assert len(tails) == len(lines) - 1 and all(t == ["0", "0"] for t in tails[0::2]) and all(int(t[1]) == 0 for t in tails)
    r = subprocess.run(base + [str(tmp_path / "m2.csv"), "256", "3"] + known, capture_output=True, text=True)
    assert r.returncode == 0 and "reseed" not in r.stdout          # without the switch the lines are what they were
    for extra in (["--known-reseed", "0"], ["--known-reseed", "1.5"], ["--known-reseed", "0.5", "0"]):
        assert subprocess.run(base + [str(tmp_path / "m3.csv"), "256", "3"] + known + extra, capture_output=True, text=True).returncode != 0
    r = subprocess.run(base + [str(tmp_path / "m4.csv"), "256", "3", "--known-reseed", "0.5"], capture_output=True, text=True)
    assert r.returncode != 0
