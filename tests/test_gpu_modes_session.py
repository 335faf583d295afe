"""slam_pf_modes on a session: PfSession.modes against the restatement (tests/_modes_spec.py) on the poses, the pending gather and the
weights the session holds (read through slam_pf_device_view just before every call, as tests/test_gpu_spread.py does) — before the
first step, after resampled and kept frames, after set_poses and reset, after a reseed; that asking changes nothing; the refusal of
sharded sessions; slam_pf_main --modes-out."""
import subprocess
import threading

import numpy as np
import pytest

import _estimate_spec as E
import _modes_spec as M
import _shard_worker as W
import test_gpu_localise_session as T
import test_gpu_spread as G
import test_gpu_spread_session as GS
from __graft_entry__ import PKG_DIR
from conftest import GOLDEN, bits

pytestmark = pytest.mark.gpu
rig = G.rig
world = GS.world
N = 4097
CELL, H, MM = 0.25, 8, 4


def _as_result(got):
    modes, cells = got
    return [M.Mode(m["pose"], m["mass"], m["cell"], m["ncells"], m["weight"]) for m in modes], cells


def _same(got, want):
    modes, cells = _as_result(got)
    return M.same(M.Result(modes, cells, want.wtotal), want)


def _check(eng, ses, fq=0, ref=0.07, tag=""):
    """modes against the restatement of the state read just before; mean and spread around it return the bits they return without it
    -> 'k' (the gate kept the last frame), 'R' (it resampled) or '|' (no frame yet)"""
    pose, anc, logw = G._state(eng, ses)
    n = pose.shape[1]
    kind, w16 = "|" if logw is None else "R", None
    if fq and logw is not None:
        w, wq = E.weights16(logw)
        if not E.gate_resamples(wq, n, fq):
            kind, w16 = "k", w
    want = M.modes_spec(pose[0], pose[1], pose[2], anc, ref, CELL, H, MM, w16)
    m0, s0 = ses.mean(ref), ses.spread(ref)
    a = ses.modes(ref, CELL, H, MM)
    b = ses.modes(ref, CELL, H, MM)
    m1, s1 = ses.mean(ref), ses.spread(ref)
    assert _same(a, want) and _same(b, want), (tag, kind, a, want)
    assert np.array_equal(bits(m0), bits(m1)) and all(np.array_equal(bits(np.asarray(p, np.float32)), bits(np.asarray(q, np.float32)))
                                                      for p, q in zip(s0, s1)), (tag, kind)
    assert sum(m.weight for m in want.modes) <= want.wtotal and (w16 is not None or want.wtotal == n)
    return kind


def test_plain_session(rig):
    x, y, th, _ = W.init_state(N, 0, rig.lm[:0])
    ses = G._session(rig, N)
    try:
        ses.set_poses(x, y, th)
        assert _check(rig.eng, ses, tag="set_poses") == "|"
        for f in range(3):
            ses.step(0, list(E.DP))
            assert _check(rig.eng, ses, ref=3.0 if f == 1 else 0.07, tag=f"frame {f}") == "R"
        ses.reset(list(E.RESET_POSE))
        assert _check(rig.eng, ses, tag="reset") == "|"
    finally:
        ses.close()


def test_gated_session_across_the_break(rig):
    """GATED_SCENARIOS' 4097: the gate's weights on the frames it kept, w = 1 elsewhere and again after the set_poses behind a kept frame"""
    sc = E.GATED_SCENARIOS[N]
    fq = E.oracle.ess_frac_q16(sc["ess"])
    x, y, th, _ = W.init_state(N, 0, rig.lm[:0])
    ses = G._session(rig, N, ess=sc["ess"], gain=sc["gain"])
    kinds = ""
    try:
        ses.set_poses(x, y, th)
        for _ in range(sc["first"]):
            ses.step(0, list(E.DP))
            kinds += _check(rig.eng, ses, fq=fq, tag=f"after {kinds}")
        assert kinds[-1] == "k"
        ses.set_poses(*(a[::-1].copy() for a in ses.poses()))
        kinds += _check(rig.eng, ses, fq=fq, tag="after the break")
        for _ in range(sc["rest"]):
            ses.step(0, list(E.DP))
            kinds += _check(rig.eng, ses, fq=fq, tag=f"after {kinds}")
    finally:
        ses.close()
    assert "k" in kinds and "R" in kinds and "k|" in kinds, kinds


def test_after_a_reseed_best_is_refused_and_modes_is_not(world):
    pkg, e, ses = T.open_session(world)
    try:
        ses.known_map_set(world["M"], T.GATE, T.CLUTTER)
        e.detections_upload(*T.detections(world, 0))
        ses.step(0, T.DP, True)
        replaced, _ = ses.known_map_reseed(0.5)
        assert replaced > 0
        with pytest.raises(pkg.SlamError) as err:
            ses.best()
        assert err.value.status == -4
        pose, anc, _ = G._state(e, ses)
        want = M.modes_spec(pose[0], pose[1], pose[2], anc, 0.0, CELL, H, MM)       # w = 1 after a reseed
        assert _same(ses.modes(0.0, CELL, H, MM), want) and want.wtotal == T.N
    finally:
        ses.close()
        e.close()


def _counters(e):
    return (e.localise_counts(), e.localise_detcov_count(), e.localise_miss_count(), e.assoc_weight_count(), e.sight_counts(), e.detect_count(),
            e.detect_fit_count(), e.detect_noise_count(), e.pose_reseed_count(), e.pose_reseed_pairs_count(), e.assoc_counts(),
            e.assoc_aniso_counts(), e.assoc_detcov_counts(), e.evidence_counts(), e.fov_counts(), e.merge_count(), e.frame_fusion_count())


def test_asking_changes_no_frame_and_no_counter(world):
    """the same known-map frames with and without modes between them: the same poses, log-weights and launch counters (the counters
    of tests/test_gpu_known_pipeline_session.py) — modes counts in none, and a session that never asks launches what it launched"""
    runs = []
    for ask in (False, True):
        pkg, e, ses = T.open_session(world, ess=T.GATE_ESS)
        ses.known_map_set(world["M"], T.GATE, T.CLUTTER)
        c0 = _counters(e)
        for f in range(T.FRAMES):
            e.detections_upload(*T.detections(world, f))
            ses.step(0, T.DP, True)
            if ask:
                ses.modes(0.0, CELL, H, MM)
        pose, anc, logw = G._state(e, ses)
        runs.append((c0, _counters(e), bits(pose).tobytes(), None if anc is None else anc.tobytes(), bits(logw).tobytes()))
        ses.close()
        e.close()
    assert runs[0] == runs[1] and runs[0][0] != runs[0][1]


def test_sharded_sessions_are_refused(rig):
    """two ranks on this card (in-process transport): INVALID_ARG on both, the status slam_pf_known_map_set gives them; nothing waits"""
    pkg = rig.pkg
    n = 256
    x, y, th, _ = W.init_state(2 * n, 0, rig.lm[:0])
    group = pkg.LocalGroup(2)
    got, errors = [None, None], []

    def rank_main(r):
        comm = None
        try:
            eng, keep = G._engine(pkg, rig.world)
            comm = pkg.Comm.local(eng, group, r)
            ses = G._session(rig, n, eng=eng, comm=comm)
            ses.set_poses(x[r * n:(r + 1) * n], y[r * n:(r + 1) * n], th[r * n:(r + 1) * n])
            try:
                ses.modes(0.0, CELL, H, MM)
            except pkg.SlamError as exc:
                got[r] = (exc.status, str(exc))
            ses.spread(0.0)            # (collective: the session is as sound as before on both ranks)
            ses.close()
            comm.close()
            eng.close()
        except BaseException as exc:   # noqa: BLE001 - re-raised below
            errors.append(exc)
            if comm:
                comm.abort()

    ths = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    group.close()
    if errors:
        raise errors[0]
    assert all(g is not None and g[0] == -2 and "sharded" in g[1] for g in got), got


def test_host_program_writes_what_the_session_returns(orc, tmp_path):
    """slam_pf_main --modes-out on the head of the recorded dataset: every line parses back to the bits PfSession.modes returns in a
    session driven from Python through the same frames; the pose log and the map are those of a run without the flag; several GPUs
    are refused."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv = GOLDEN / "frames_head.csv"
    lines = csv.read_text().splitlines()
    base = [str(exe), str(csv), str(len(lines)), str(len(lines[0].split(",")))]
    args = ["--modes-out", str(tmp_path / "modes.txt"), "0.05", "16", "3"]

    def run(tag, *extra):
        r = subprocess.run(base + [str(tmp_path / f"map_{tag}.csv"), str(GS.HOST_N), str(GS.HOST_SEED)] + list(extra), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout, (tmp_path / f"map_{tag}.csv").read_bytes()

    plain = run("plain")
    assert run("flag", *args) == plain
    want = []

    def configure(pkg, e, ses, ang):
        spread = ses.spread

        def spread_and_modes(ref):
            want.append(ses.modes(ref, 0.05, 16, 3))
            return spread(ref)
        ses.spread = spread_and_modes

    log, _, _ = GS.python_run(orc, csv, 0.0, configure=configure)
    assert log == plain[0]
    got = (tmp_path / "modes.txt").read_text().splitlines()
    assert len(got) == len(want) == len(lines) - 1
    for k, (ln, (modes, cells)) in enumerate(zip(got, want)):
        t = ln.split(" ")
        assert (int(t[0]), int(t[1]), int(t[2])) == (k + 2, len(modes), cells) and len(t) == 3 + 4 * len(modes), ln
        v = np.array([float(u) for u in t[3:]], np.float32)
        assert [f"{float(u):.9g}" for u in v] == t[3:], ln
        flat = np.concatenate([np.append(m["pose"], m["mass"]) for m in modes]).astype(np.float32)
        assert np.array_equal(bits(v), bits(flat)), (ln, modes)
        assert 1 <= len(modes) <= 3
    r = subprocess.run(base + [str(tmp_path / "m2.csv"), str(GS.HOST_N), str(GS.HOST_SEED), "--gpus", "2", "--transport", "local", "--same-device"]
                       + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--modes-out" in r.stderr and "pose =" not in r.stdout
