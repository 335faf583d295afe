"""slam_pf_known_map_reseed_pairs inside a session against the frame loop of tests/_reseed_pair_spec.py: 256 particles, 12 landmarks,
8 frames, in both noise forms (and ESS-gated) — poses after every frame and after every reseed bit for bit, log-weights, ancestors
and verdicts of every frame, the four counts; two calls with no step between them; slam_pf_best refused from the call to the next
step; a session that never calls it runs the launches it ran; the refusals; and slam_pf_main --known-reseed-pairs."""
import subprocess

import numpy as np
import pytest
import torch

import _localise_detcov_spec as SD
import _localise_spec as S
import _reseed_pair_spec as RP
import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import GOLDEN, bits
from test_gpu_localise_session import compare, frame
from test_gpu_reseed_session import CLUTTER, DP, GATE, GATE_ESS, KW, detections, hand_over, spec_kw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES = 256, 12, 8
TOL, MIN_SEP = 0.05, 0.5
FRACTIONS = {1: 0.25, 2: 1.0 / 16, 4: 1.0, 5: 0.5, 6: 2.0**-10}   # frame -> the fraction reseeded behind it
NOT_READY, INVALID_ARG = -4, -2


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, bx, by, lm = W.make_world(L=L)
    x, y, th, _ = W.init_state(N, 0, np.zeros((0, 2), np.float32))
    M = np.zeros((5, L), np.float32)
    M[0], M[1], M[2], M[4] = lm[:, 0], lm[:, 1], 0.05, 0.05
    M[3] = 0.01
    M[2, ::5] = -1.0                             # slots that hold no landmark
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), bx=bx, by=by, lm=lm, x=x, y=y, th=th, M=M)


def reference(world, detcov, ess, reseed_after):
    return RP.frame_loop(world, N, FRAMES, dp=DP, detections=lambda f: detections(world, f, detcov), known_map=world["M"], gate=GATE,
                         log_clutter=CLUTTER, ess=ess, reseed_after=reseed_after, tol=TOL, min_sep=MIN_SEP, **spec_kw(detcov))


def open_session(world, ess=0.0, **kw):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    ses = pkg.PfSession(e, N, kw.pop("n_landmarks", 0), resample_ess_frac=ess, **kw, **KW)
    ses.set_poses(world["x"], world["y"], world["th"])
    return pkg, e, ses


def launch_counters(e):
    """the existing counters a frame of a known-map session moves, and the two reseeds'"""
    return dict(localise=e.localise_counts(), detcov=e.localise_detcov_count(), miss=e.localise_miss_count(), single=e.pose_reseed_count(),
                pairs=e.pose_reseed_pairs_count())


@pytest.mark.parametrize("detcov", [False, True], ids=["meas-var", "per-detection"])
@pytest.mark.parametrize("ess", [0.0, GATE_ESS], ids=["every-frame", "gated"])
def test_session_equals_the_spec_loop(world, ess, detcov):
    want = reference(world, detcov, ess, FRACTIONS.get)
    counts = {f: tuple(int(v) for v in want[f]["counts"]) for f in FRACTIONS}
    print("counts", counts)
    assert sum(counts[4]) == N and all(c[0] > 0 for f, c in counts.items() if f != 6) and counts[4][1] > 0
    pkg, e, ses = open_session(world, ess=ess)
    (ses.known_map_detcov_set if detcov else ses.known_map_set)(world["M"], GATE, CLUTTER)
    c0 = launch_counters(e)
    for f in range(FRAMES):
        hand_over(e, world, f, detcov)
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f}")
        best = ses.best()
        if f in FRACTIONS:
            assert ses.known_map_reseed_pairs(FRACTIONS[f], TOL, MIN_SEP) == counts[f], f"frame {f}: counts"
            assert ses.device_view()["anc"] is None
            got = ses.poses()
            assert np.array_equal(bits(got), bits(want[f]["reseeded"])), f"frame {f}: the reseeded population"
            with pytest.raises(pkg.SlamError, match="reseeded") as err:
                ses.best()
            assert err.value.status == NOT_READY
            if f in (1, 4):   # no step in between: the same draws, now without a pending gather — the same population again
                again = RP.reseed_pairs(world["M"], *got, None, *detections(world, f, False), 0, KW["seed"], f + 1, FRACTIONS[f], TOL, MIN_SEP)
                assert ses.known_map_reseed_pairs(FRACTIONS[f], TOL, MIN_SEP) == tuple(again[4]) == counts[f]
                assert np.array_equal(bits(ses.poses()), bits(np.stack(again[:3])))
                replaced = again[3] == 1          # a proposal does not depend on the pose it replaces: it lands where it landed
                assert np.array_equal(bits(np.stack(again[:3])[:, replaced]), bits(got[:, replaced]))
                if FRACTIONS[f] == 1.0:           # ... and the slots that were not replaced kept their own pose: the same population
                    assert np.array_equal(bits(ses.poses()), bits(got))
        else:
            assert best[2] == int(np.argmax(want[f]["logw"]))
    c1 = launch_counters(e)
    assert c1["pairs"] - c0["pairs"] == len(FRACTIONS) + 2 and c1["single"] == c0["single"]
    if ess:
        verdicts = [w["resampled"] for w in want]
        assert ses.frames_resampled() == sum(verdicts[:-1])   # the host has looked at every frame but the last
    ses.close()
    e.close()


@pytest.mark.parametrize("detcov", [False, True], ids=["meas-var", "per-detection"])
def test_a_session_that_never_calls_it_runs_the_launches_it_ran(world, detcov):
    det = lambda f: detections(world, f, detcov)
    common = dict(dp=DP, detections=det, known_map=world["M"], gate=GATE, log_clutter=CLUTTER, **spec_kw(detcov))
    want = (SD if detcov else S).frame_loop(world, N, FRAMES, **common)
    mine = RP.frame_loop(world, N, FRAMES, tol=TOL, min_sep=MIN_SEP, **common)   # the extended loop without a reseed IS the unextended one
    pkg, e, ses = open_session(world)
    (ses.known_map_detcov_set if detcov else ses.known_map_set)(world["M"], GATE, CLUTTER)
    c0 = launch_counters(e)
    for f in range(FRAMES):
        assert all(np.array_equal(bits(mine[f][k]), bits(want[f][k])) for k in ("pose", "logw")) and np.array_equal(mine[f]["anc"], want[f]["anc"])
        hand_over(e, world, f, detcov)
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f}")
        assert ses.best()[2] == int(np.argmax(want[f]["logw"]))
    c1 = launch_counters(e)
    # one localise launch a frame in the session's own noise form, as before; nothing else moved
    stage = (c1["detcov"] - c0["detcov"]) if detcov else (c1["localise"][1] - c0["localise"][1])
    assert stage == FRAMES and c1["pairs"] == c0["pairs"] and c1["single"] == c0["single"] and c1["miss"] == c0["miss"]
    ses.close()
    e.close()


def test_refusals_leave_the_session_as_it_was(world):
    pkg = load_package()

    def refused(ses, text, status=NOT_READY, fraction=0.5, tol=TOL, min_sep=MIN_SEP):
        with pytest.raises(pkg.SlamError, match=text) as err:
            ses.known_map_reseed_pairs(fraction, tol, min_sep)
        assert err.value.status == status

    want = reference(world, False, 0.0, None)
    _, e, ses = open_session(world)
    c0 = e.pose_reseed_pairs_count()
    hand_over(e, world, 0, False)
    refused(ses, "mode is off")
    ses.known_map_set(world["M"], GATE, CLUTTER)
    for bad in (0.0, -1.0, 1.5, float("nan")):
        refused(ses, "fraction", status=INVALID_ARG, fraction=bad)
    for tol, sep in ((-0.1, 1.0), (float("nan"), 1.0), (0.5, 0.5), (0.5, 0.25), (0.0, float("inf")), (0.0, float("nan")), (float("inf"), float("inf"))):
        refused(ses, "tol", status=INVALID_ARG, tol=tol, min_sep=sep)
    for f in range(2):
        hand_over(e, world, f, False)
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f}")
        for K in (0, 1):   # fewer than two detections: nothing happens, the gather stays pending, best still answers
            e.detections_upload(np.ones(K, np.float32), np.ones(K, np.float32))
            assert ses.known_map_reseed_pairs(1.0, TOL, MIN_SEP) == (0, 0, 0, 0)
            assert ses.device_view()["anc"] is not None and ses.best()[2] == int(np.argmax(want[f]["logw"]))
    ses.known_map_set(None)
    refused(ses, "mode is off")
    assert e.pose_reseed_pairs_count() == c0
    ses.close()
    e.close()

    _, e, ses = open_session(world, n_landmarks=8, map_layout="rows")
    hand_over(e, world, 0, False)
    refused(ses, "n_landmarks > 0")
    ses.close()
    e.close()

    _, e, ses = open_session(world)   # a known map, and no detections were ever handed over
    ses.known_map_set(world["M"], GATE, CLUTTER)
    refused(ses, "no detections")
    ses.known_map_set(world["M"][:, :1], GATE, CLUTTER)   # a map of one landmark has no pair
    refused(ses, "two landmarks", status=INVALID_ARG)
    ses.close()
    e.close()


def test_host_program_reseeds_from_pairs(orc, tmp_path):
    """slam_pf_main --known-map --known-reseed-pairs on the head of the recorded dataset: every frame's line carries the four
    counts, which add up to the population or, where the detector found fewer than two poles (the frame is skipped), to nothing;
    only every second frame with EVERY = 2; refused with --known-reseed, without --known-map and with bad parameters."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv = GOLDEN / "frames_head.csv"
    lines = csv.read_text().splitlines()
    base = [str(exe), str(csv), str(len(lines)), str(len(lines[1].split(",")))]
    km = tmp_path / "known.csv"
    km.write_text("".join(f"{x:f},{y:f}\n" for x, y in np.random.default_rng(3).uniform(-8, 8, (20, 2))))
    known = ["--known-map", str(km), "9.21", "0.05", "-2.5", "--detect"]
    r = subprocess.run(base + [str(tmp_path / "m0.csv"), "256", "3"] + known + ["--known-reseed-pairs", "1", "0.1", "0.5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tails = [[int(v) for v in ln.split("reseed-pairs = ")[1].split()] for ln in r.stdout.splitlines() if ln.startswith("pose =")]
    assert len(tails) == len(lines) - 1 and all(len(t) == 4 and sum(t) in (0, 256) for t in tails)
    r = subprocess.run(base + [str(tmp_path / "m1.csv"), "256", "3"] + known + ["--known-reseed-pairs", "0.5", "0.1", "0.5", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tails = [[int(v) for v in ln.split("reseed-pairs = ")[1].split()] for ln in r.stdout.splitlines() if ln.startswith("pose =")]
    assert len(tails) == len(lines) - 1 and all(sum(t) == 0 for t in tails[0::2])
    for extra in (["--known-reseed-pairs", "0", "0.1", "0.5"], ["--known-reseed-pairs", "0.5", "0.5", "0.5"], ["--known-reseed-pairs", "0.5", "-1", "0.5"],
                  ["--known-reseed-pairs", "0.5", "0.1", "0.5", "0"], ["--known-reseed-pairs", "0.5", "0.1", "0.5", "--known-reseed", "0.5"]):
        assert subprocess.run(base + [str(tmp_path / "m3.csv"), "256", "3"] + known + extra, capture_output=True, text=True).returncode != 0
    r = subprocess.run(base + [str(tmp_path / "m4.csv"), "256", "3", "--known-reseed-pairs", "0.5", "0.1", "0.5"], capture_output=True, text=True)
    assert r.returncode != 0
