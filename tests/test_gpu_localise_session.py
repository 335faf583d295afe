"""A session without maps of its own that localises in ONE known landmark map (slam_pf_known_map_set) against the frame loop of
tests/_localise_spec.py, frame by frame and bit for bit: poses, log-weights, ancestors, the resample verdicts and the stage's
stats — resampling every frame and ESS-gated, refining, with uploaded detections and with the detector, with and without a clutter
term; switched off mid-run; frames without observations; every refusal; the launch counters; and slam_pf_main --known-map."""
import subprocess

import numpy as np
import pytest
import torch

import _detect_scenes as DS
import _detect_spec as D
import _localise_spec as S
import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import GOLDEN, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES, K = 256, 40, 6, 24
GATE, CLUTTER = 9.21, -2.5
GATE_ESS = 0.5
REFINE = (0.05, 0.008727, 1)
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
DP = [0.01, -0.005, 0.002]


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, bx, by, lm = W.make_world(L=L)
    x, y, th, _ = W.init_state(N, 0, np.zeros((0, 2), np.float32))
    M = np.zeros((5, L), np.float32)
    M[0], M[1], M[2], M[4] = lm[:, 0], lm[:, 1], 0.05, 0.05
    M[3] = 0.01
    M[2, ::7] = -1.0                             # slots that hold no landmark, scattered through the map
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), bx=bx, by=by, lm=lm, x=x, y=y, th=th, M=M)


def detections(world, f):
    """24 of the world's landmark observations of frame f, in shuffled order and without their ids."""
    _, zx, zy = W.observations(world["lm"], 0)
    zx, zy = zx + np.float32(0.01 * f), zy + np.float32(0.01 * f)
    pick = np.random.default_rng(100 + f).permutation(len(zx))[:K]
    return zx[pick].copy(), zy[pick].copy()


def reference(world, known_map, frames=FRAMES, ess=0.0, refine=None, clutter=CLUTTER, det=None, scans=None):
    return S.frame_loop(world, N, frames, dp=DP, detections=det or (lambda f: detections(world, f)), known_map=known_map, gate=GATE,
                        log_clutter=clutter, ess=ess, refine=refine, scans=scans, **KW)


def open_session(world, ess=0.0, refine=None, layout=None, n_landmarks=0):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    ses = pkg.PfSession(e, N, n_landmarks, resample_ess_frac=ess, map_layout=layout, **KW)
    if refine:
        ses.refine_set(*refine)
    ses.set_poses(world["x"], world["y"], world["th"])
    return pkg, e, ses


def frame(e, ses, stats=True):
    v = ses.device_view()
    e.sync()
    fr = dict(pose=ses.poses(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
              anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy() if v["anc"] is not None else None)
    if stats:
        fr["stats"] = torch.as_tensor(ses.known_map_view()["stats"], device=DEV).cpu().numpy()
    return fr


def compare(g, w, label):
    if w["stats"] is not None and "stats" in g:
        assert np.array_equal(g["stats"], w["stats"]), f"{label}: stats"
    assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label}: log-weights"
    ga, wa = (np.arange(len(w["logw"])) if a is None else a for a in (g["anc"], w["anc"]))
    assert np.array_equal(ga, wa), f"{label}: ancestors"
    assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label}: poses"


@pytest.mark.parametrize("clutter", [CLUTTER, 0.0], ids=["clutter", "no-clutter"])
@pytest.mark.parametrize("refine", [None, REFINE], ids=["plain", "refined"])
@pytest.mark.parametrize("ess", [0.0, GATE_ESS], ids=["every-frame", "gated"])
def test_session_equals_the_spec_loop(world, ess, refine, clutter):
    want = reference(world, world["M"], ess=ess, refine=refine, clutter=clutter)
    st = np.stack([w["stats"] for w in want])
    assert st[..., 0].sum() > 0 and st[..., 2].sum() > 0 and np.all(st[..., 1] == 0)   # matches and unmatched detections
    verdicts = [w["resampled"] for w in want]
    pkg, e, ses = open_session(world, ess=ess, refine=refine)
    c0, w0 = e.localise_counts(), e.assoc_weight_count()
    ses.known_map_set(world["M"], GATE, clutter)
    for f in range(FRAMES):
        e.detections_upload(*detections(world, f))
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f}")
    assert ses.frames_resampled() == (sum(verdicts[:-1]) if ess else 0)   # the host has looked at every frame but the last
    assert tuple(np.subtract(e.localise_counts(), c0)) == (1, FRAMES)      # one prepare launch per set, one stage launch per frame
    assert e.assoc_weight_count() - w0 == (FRAMES if clutter else 0)
    v = ses.known_map_view()
    assert v["nlandmarks"] == L and v["prepared"] is not None
    ses.close()
    e.close()


def scans_and_map():
    """Another pole field every frame; the known map: what the detector sees in the first two of them from the origin (H = I:
    the world point is the sensor point), the rest of the slots empty."""
    scans, kws = [], None
    for f in range(FRAMES):
        bx, by, kws = DS.pole_field(360, 30 + f)
        scans.append((bx, by))
    M = np.zeros((5, L), np.float32)
    M[2] = -1.0
    pts = []
    for f in (0, 1):
        zx, zy, k, _ = D.detect(*scans[f], **kws)
        pts += [(zx[j], zy[j]) for j in range(k)]
    pts = pts[:L - 5]
    for j, (px, py) in enumerate(pts):
        M[:, j + 2] = (px, py, 0.05, 0.0, 0.08)
    return scans, kws, M


def test_session_with_the_detector_equals_the_spec_loop(world):
    scans, kws, M = scans_and_map()

    def det(f):
        zx, zy, k, _ = D.detect(*scans[f], **kws)
        return zx[:k].copy(), zy[:k].copy()

    want = reference(world, M, det=det, scans=scans)
    assert min(len(det(f)[0]) for f in range(FRAMES)) >= 3 and sum(int(w["stats"][:, 0].sum()) for w in want) > 0
    pkg, e, ses = open_session(world)
    ses.known_map_set(M, GATE, CLUTTER)
    ses.detect_set(pkg.DetectParams.default(**kws))
    with pytest.raises(pkg.SlamError, match="meas_var"):
        ses.detect_noise_set((0.01, 0.0001, 0.0))
    d0, c0 = e.detect_count(), e.localise_counts()
    for f in range(FRAMES):
        e.scan_upload(*scans[f])
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f}")
    assert e.detect_count() - d0 == FRAMES and tuple(np.subtract(e.localise_counts(), c0)) == (0, FRAMES)
    ses.close()
    e.close()


def test_switched_off_and_frames_without_observations(world):
    """Frames 0, 1 and 3 localise, frame 2 has use_observations = 0, in front of frame 4 the mode is switched off: from there on,
    and in frame 2, the session runs the frame of one that never had the mode — the spec loop's plain frame from the same state
    (plain weights) — and launches no stage."""
    observing = lambda f: f != 2
    want = reference(world, lambda f: world["M"] if f < 4 else None, det=lambda f: detections(world, f) if observing(f) else None)
    pkg, e, ses = open_session(world)
    ses.known_map_set(world["M"], GATE, CLUTTER)
    c0, w0 = e.localise_counts(), e.assoc_weight_count()
    for f in range(FRAMES):
        if f == 4:
            ses.known_map_set(None)
            assert ses.known_map_view()["prepared"] is None
        e.detections_upload(*detections(world, f))
        ses.step(0, DP, observing(f))
        compare(frame(e, ses, stats=False), want[f], f"frame {f}")
    assert tuple(np.subtract(e.localise_counts(), c0)) == (0, 3) and e.assoc_weight_count() - w0 == 3
    ses.close()
    e.close()


def plain_frame(world, ask=None, comm_group=None, **kw):
    """The first frame (no observations) of a fresh session; ask(pkg, ses): called on it first."""
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    comm = pkg.Comm.local(e, comm_group, 0) if comm_group else None
    ses = pkg.PfSession(e, N, comm=comm, **kw, **KW)
    ses.set_poses(world["x"], world["y"], world["th"])
    if ask:
        ask(pkg, ses)
    ses.step(0, DP, False)
    v = ses.device_view()
    e.sync()
    out = ses.poses(), torch.as_tensor(v["logw"], device=DEV).cpu().numpy(), e.localise_counts()
    ses.close()
    if comm:
        comm.close()
    e.close()
    return out


def test_refusals_leave_the_session_as_it_was(world):
    """Every refusal says SLAM_ERR_INVALID_ARG and why; on a session that has a map set the next frame is the spec's frame with
    THAT map; a session with landmarks of its own and a sharded one run the frame of a session that was never asked."""
    pkg = load_package()
    M = world["M"]

    def changed(*edits):
        B = M.copy()
        for p, l, v in edits:
            B[p, l] = v
        return B

    def raw(ses, nlandmarks):   # (the binding takes the number of landmarks from the array)
        rc = ses.e.lib.slam_pf_known_map_set(ses.h, M.ctypes.data, nlandmarks, GATE, 0.0)
        raise pkg.SlamError(rc, "pf_known_map_set", ses.e.lib.slam_last_error(ses.e.h).decode())

    calls = [("landmarks", lambda s: raw(s, 0)), ("landmarks", lambda s: raw(s, 8193)),
             ("gate", lambda s: s.known_map_set(M, 0.0, 0.0)), ("gate", lambda s: s.known_map_set(M, float("inf"), 0.0)),
             ("gate", lambda s: s.known_map_set(M, float("nan"), 0.0)), ("gate", lambda s: s.known_map_set(M, -1.0, 0.0)),
             ("log_clutter", lambda s: s.known_map_set(M, GATE, 0.5)), ("log_clutter", lambda s: s.known_map_set(M, GATE, float("nan"))),
             ("log_clutter", lambda s: s.known_map_set(M, GATE, -float("inf"))),
             ("not finite", lambda s: s.known_map_set(changed((0, 1, np.nan)), GATE, 0.0)),
             ("not finite", lambda s: s.known_map_set(changed((4, 2, np.inf)), GATE, 0.0)),
             ("positive definite", lambda s: s.known_map_set(changed((4, 3, -0.5)), GATE, 0.0)),      # P_yy + q <= 0
             ("positive definite", lambda s: s.known_map_set(changed((3, 4, 10.0)), GATE, 0.0))]      # det S <= 0
    want = reference(world, M, frames=1)[0]
    _, e, ses = open_session(world)
    ses.known_map_set(M, GATE, CLUTTER)
    c0 = e.localise_counts()
    for text, call in calls:
        with pytest.raises(pkg.SlamError, match=text) as err:
            call(ses)
        assert err.value.status == -2, text   # SLAM_ERR_INVALID_ARG
    assert e.localise_counts() == c0
    e.detections_upload(*detections(world, 0))
    ses.step(0, DP, True)
    compare(frame(e, ses), want, "after the refusals")
    ses.close()
    e.close()

    def refused(pkg, ses):
        with pytest.raises(pkg.SlamError, match="n_landmarks == 0") as err:
            ses.known_map_set(M, GATE, CLUTTER)
        assert err.value.status == -2

    group = pkg.LocalGroup(1)
    for label, kw in (("landmarks", dict(n_landmarks=8, map_layout="rows")), ("sharded", dict(comm_group=group))):
        plain, asked = plain_frame(world, **kw), plain_frame(world, ask=refused, **kw)
        assert np.array_equal(bits(plain[0]), bits(asked[0])) and np.array_equal(bits(plain[1]), bits(asked[1])), label
        assert asked[2] == (0, 0), label
    group.close()


def test_host_program_localises_in_a_known_map(orc, tmp_path):
    """slam_pf_main --known-map on the head of the recorded dataset runs to completion; the forbidden combinations exit non-zero."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv = GOLDEN / "frames_head.csv"
    lines = csv.read_text().splitlines()
    base = [str(exe), str(csv), str(len(lines)), str(len(lines[1].split(",")))]
    km = tmp_path / "known.csv"
    km.write_text("".join(f"{x:f},{y:f}\n" for x, y in np.random.default_rng(3).uniform(-8, 8, (20, 2))))
    known = ["--known-map", str(km), "9.21", "0.05"]
    r = subprocess.run(base + [str(tmp_path / "m0.csv"), "256", "3"] + known + ["-2.5", "--detect"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("pose =") == len(lines) - 1, r.stderr
    r = subprocess.run(base + [str(tmp_path / "m1.csv"), "256", "3"] + known + ["--detect", "--pole-radius", "0.1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("pose =") == len(lines) - 1, r.stderr
    for extra in (["--landmarks", "16"], ["--gpus", "2", "--transport", "local", "--same-device"], ["--meas-cov", "0.02", "0", "0.03"]):
        r = subprocess.run(base + [str(tmp_path / "m2.csv"), "256", "3"] + known + ["--detect"] + extra, capture_output=True, text=True)
        assert r.returncode != 0, extra
    r = subprocess.run(base + [str(tmp_path / "m3.csv"), "256", "3", "--known-map", str(tmp_path / "missing.csv"), "9.21", "0.05"],
                       capture_output=True, text=True)
    assert r.returncode != 0
