"""A rows session with EVERY switch of the associating frame against the composed frame loop of tests/_pipeline_spec.py, over the
twelve frames of tests/_pipeline_scenes.py, bit for bit and frame by frame: poses, map rows, log-weights, ancestors, the
association table, evidence bytes and stats, spared and outside counts, merge stats (and the detector's detections and
covariances) — eight combinations of noise form, detector form, evidence stage, merging, refinement and resample gate, the last
but two of them the whole pipeline; the launch counters of every stage, on or off; switches changed in the middle of a run, the
noise form given anew among them; slam_pf_assoc_set(0) with everything switched on again; and slam_pf_main with every option."""
import json
import subprocess

import numpy as np
import pytest
import torch

import _pipeline_scenes as SC
import _pipeline_spec as P
from __graft_entry__ import PKG_DIR, load_package
from conftest import GOLDEN, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES = SC.N, SC.L, SC.FRAMES


@pytest.fixture(scope="module")
def world(orc):
    w = SC.make_world()
    return dict(w, d_edt=torch.from_numpy(w["edt"]).to(DEV))


def switch_noise(ses, noise):
    if noise[0] == "iso":
        ses.assoc_set(SC.GATE, SC.NEW_GATE, True)
    elif noise[0] == "cov":
        ses.assoc_cov_set(noise[1], SC.GATE, SC.NEW_GATE, True)
    else:
        ses.assoc_detcov_set(SC.GATE, SC.NEW_GATE, True)


def switch_rest(ses, kw):
    """Everything that hangs on association, in the order a caller would give it."""
    if kw.get("prune"):
        ses.prune_set(*kw["prune"])
    if kw.get("sight"):
        ses.prune_sight_set(*kw["sight"])
    if kw.get("fov"):
        ses.prune_fov_set(True, *SC.ARC)
    if kw.get("merge_gate"):
        ses.merge_set(kw["merge_gate"])
    d = kw.get("detector")
    if d:
        ses.detect_noise_set(d.get("noise"), d.get("fit"), **d["params"])


def open_session(world, kw):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    ses = pkg.PfSession(e, N, L, resample_ess_frac=kw.get("ess", 0.0), map_layout="rows", **SC.KW)
    if kw.get("refine"):
        ses.refine_set(*kw["refine"])
    switch_noise(ses, kw.get("noise", ("iso",)))
    ses.set_poses(world["x"], world["y"], world["th"])
    ses.set_map(world["mp"])
    switch_rest(ses, kw)
    return e, ses


def hand_over(e, f, kw, cov=None):
    """The frame's scan, and (no detector) its detections; cov: upload the covariances (default: where the hand-over has them)."""
    e.scan_upload(*SC.SCANS[f])
    if kw.get("detector"):
        return
    det = kw["detections"](f)
    e.detections_upload(det[0], det[1])
    if len(det) == 3 and cov is not False:
        e.detections_cov_upload(*det[2])


def host(a):
    return torch.as_tensor(a, device=DEV).cpu().numpy()


def frame(e, ses, kw):
    """What the session holds behind a frame; kw: the switches in force in that frame."""
    v, av = ses.device_view(), ses.assoc_view()
    e.sync()
    fr = dict(pose=ses.poses(), map=ses.maps(), logw=host(v["logw"]), anc=host(v["anc"]), assoc=host(av["assoc"]), stats=host(av["stats"]))
    if kw.get("prune"):
        fr["ev"] = ses.evidence()
        fr["ev_stats"] = host(ses.evidence_view()["stats"])
        if kw.get("sight"):
            fr["spared"] = host(ses.sight_view()["spared"])
        if kw.get("fov"):
            fr["outside"] = host(ses.fov_view()["outside"])
    if kw.get("merge_gate"):
        fr["merge_stats"] = host(ses.merge_view())
    if kw.get("detector"):
        fr["det"] = e.detections() + ((e.detections_cov(),) if kw["detector"].get("noise") else ())
    return fr


def compare(g, w, label):
    assert np.array_equal(g["assoc"][:, :L], w["assoc"]) and np.all(g["assoc"][:, L:] == 255), f"{label}: association table"
    assert np.array_equal(g["stats"], w["stats"]), f"{label}: association stats"
    assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label}: log-weights"
    assert np.array_equal(g["anc"], w["anc"]), f"{label}: ancestors"
    assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label}: poses"
    assert np.array_equal(bits(g["map"]), bits(w["map"])), f"{label}: map rows"
    for k in ("ev", "ev_stats", "spared", "outside", "merge_stats"):
        if k in g:
            assert w[k] is not None and np.array_equal(g[k], w[k]), f"{label}: {k}"
    if "det" in g:
        zx, zy, q = w["det"]
        assert np.array_equal(bits(g["det"][0]), bits(zx)) and np.array_equal(bits(g["det"][1]), bits(zy)), f"{label}: detections"
        if len(g["det"]) == 3:
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(g["det"][2], q)), f"{label}: the detections' covariances"


def counters(e):
    return dict(merge=e.merge_count(), evidence=e.evidence_counts(), sight=e.sight_counts(), fov=e.fov_counts(), iso=e.assoc_counts(),
                cov=e.assoc_aniso_counts(), detcov=e.assoc_detcov_counts(), detect=e.detect_count(), fit=e.detect_fit_count(),
                model=e.detect_noise_count(), forms=e.ekf_form_counts(), inplace=e.ekf_inplace_form_counts(), aniso=e.ekf_aniso_count(),
                fused=e.frame_fusion_count())


def advance(e, c0):
    c1 = counters(e)
    return {k: tuple(np.subtract(c1[k], c0[k]).tolist()) if isinstance(c1[k], tuple) else c1[k] - c0[k] for k in c1}


def expected(kw, frames):
    """Every stage that is on: once per observing frame, in its own counter; every stage that is off: not at all."""
    pr, sg, fv, d = kw.get("prune"), kw.get("sight"), kw.get("fov"), kw.get("detector") or {}
    form = kw.get("noise", ("iso",))[0]
    n = lambda on: frames if on else 0
    return dict(merge=n(kw.get("merge_gate")), evidence=(n(pr and not sg and not fv), 0), sight=(n(pr and sg), n(pr and sg and not fv)),
                fov=n(pr and fv), iso=(n(form == "iso"),) * 2, cov=(n(form == "cov"),) * 2, detcov=(n(form == "detcov"),) * 2,
                detect=n(d), fit=n(d.get("fit")), model=n(d.get("noise")), forms=(0, 0), inplace=(0, 0), aniso=0, fused=0)


@pytest.mark.parametrize("name", list(SC.COMBOS))
def test_session_equals_the_composed_loop(world, name):
    kw = SC.COMBOS[name]
    e, ses = open_session(world, kw)
    fov = None
    if kw.get("fov"):                            # the bounds the library's cosine and sine gave: the spec's from here on
        fov = ses.fov_view()["bounds"]
        assert all(abs(float(a) - float(b)) < 1e-6 for a, b in zip(fov, SC.bounds()))
    SC.check_not_vacuous(world, name, fov)
    want = SC.reference(world, name, fov)
    c0 = counters(e)
    for f in range(FRAMES):
        hand_over(e, f, kw)
        ses.step(0, SC.DP, True)
        compare(frame(e, ses, kw), want[f], f"{name}: frame {f}")
    assert advance(e, c0) == expected(kw, FRAMES)
    if kw.get("ess"):
        assert ses.frames_resampled() == sum(w["resampled"] for w in want[:-1])   # the host has looked at every frame but the last
    ses.step(0, SC.DP, False)                    # a frame without a detection hand-over runs none of the stages
    assert advance(e, c0) == expected(kw, FRAMES)
    ses.close()
    e.close()


# ------------------------------------------------------------------ switches in the middle of a run
SWITCHING = dict(detections=SC.with_cov, prune=SC.PRUNE,
                 noise=lambda f: ("iso",) if f < 5 else ("cov", SC.COV) if f < 8 else ("detcov",),
                 sight=lambda f: SC.SIGHT if f >= 3 else None, fov=lambda f: True if f >= 3 else None,
                 merge_gate=lambda f: SC.MERGE_GATE if f < 10 else 0.0)


def at(kw, f):
    return {k: (v(f) if callable(v) and k != "detections" else v) for k, v in kw.items()}


def switching_reference(world, fov, restart=()):
    kw = dict(SWITCHING, fov=lambda f: tuple(fov) if f >= 3 else None)
    return P.frame_loop(world, SC.SCANS, N, FRAMES, dp=SC.DP, gate=SC.GATE, new_gate=SC.NEW_GATE, create=1, restart=restart, **kw, **SC.KW)


def test_switching_mid_run(world):
    """Isotropic with pruning and merging; line of sight and field of view from frame 3; the noise form given anew at frame 5
    (slam_pf_assoc_cov_set) and at frame 8 (slam_pf_assoc_detcov_set, covariances uploaded from there on); merging off at frame 10.
    A noise form given anew leaves pruning and its evidence bytes, line of sight, field of view and merging as they were."""
    e, ses = open_session(world, at(SWITCHING, 0))
    ses.prune_fov_set(True, *SC.ARC)
    fov = ses.fov_view()["bounds"]
    ses.prune_fov_set(False)
    want = switching_reference(world, fov)
    # the reference alone: every span of the run holds what its switches react to, and evidence that had been initialised anew
    # at either change of the noise form would show
    span = lambda k, a, b, col=None: sum(int((w[k] if col is None else w[k][:, col]).sum()) for w in want[a:b] if w[k] is not None)
    assert all(w["spared"] is None and w["outside"] is None for w in want[:3]) and all(w["merge_stats"] is None for w in want[10:])
    for a, b in ((5, 8), (8, 10)):               # behind either change of the noise form
        assert span("spared", a, b) > 0 and span("outside", a, b) > 0 and span("merge_stats", a, b, 0) > 0, (a, b)
    assert span("merge_stats", 0, 3, 0) > 0 and span("spared", 3, 5) > 0 and span("merge_stats", 3, 5, 0) > 0
    assert span("ev_stats", 5, 12, 0) > 0 and span("outside", 10, 12) > 0
    anew = switching_reference(world, fov, restart=(5, 8))
    assert not np.array_equal(anew[5]["ev"], want[5]["ev"]) and not np.array_equal(anew[8]["ev"], want[8]["ev"])
    c0 = counters(e)
    for f in range(FRAMES):
        if f == 3:
            ses.prune_sight_set(*SC.SIGHT)
            ses.prune_fov_set(True, *SC.ARC)
        if f in (5, 8):
            switch_noise(ses, SWITCHING["noise"](f))
        if f == 10:
            ses.merge_set(0.0)
        kw = at(SWITCHING, f)
        hand_over(e, f, kw, cov=f >= 8)
        ses.step(0, SC.DP, True)
        compare(frame(e, ses, kw), want[f], f"switching: frame {f}")
    assert advance(e, c0) == dict(merge=10, evidence=(3, 0), sight=(9, 0), fov=9, iso=(5, 5), cov=(3, 3), detcov=(4, 4), detect=0, fit=0,
                                  model=0, forms=(0, 0), inplace=(0, 0), aniso=0, fused=0)
    ses.close()
    e.close()


def test_association_off_and_everything_on_again(world):
    """slam_pf_assoc_set(0) in front of frame 6 clears every switch that hangs on association — given a noise form alone behind
    it, a frame runs the association's two stages and nothing else.  With all the switches given again the run goes on as a
    fresh session's would from that frame's poses and maps: evidence from the maps, everything else as it was."""
    name = "uploaded+Qk detcov sight+fov"
    kw = SC.COMBOS[name]
    pkg = load_package()
    e, ses = open_session(world, kw)
    fov = ses.fov_view()["bounds"]
    want = P.frame_loop(world, SC.SCANS, N, FRAMES, dp=SC.DP, gate=SC.GATE, new_gate=SC.NEW_GATE, create=1, restart=(6,),
                        **dict(kw, fov=tuple(fov)), **SC.KW)
    straight = SC.reference(world, name, fov)
    assert not np.array_equal(want[6]["ev"], straight[6]["ev"])                      # (the evidence that is lost shows)
    for f in range(FRAMES):
        if f == 6:
            ses.assoc_set(0.0)
            with pytest.raises(pkg.SlamError):
                ses.merge_set(SC.MERGE_GATE)                                            # (nothing hangs on an association that is off)
            switch_noise(ses, kw["noise"])
            switch_rest(ses, kw)
        hand_over(e, f, kw)
        ses.step(0, SC.DP, True)
        compare(frame(e, ses, kw), want[f], f"restart: frame {f}")
    # ... and a noise form alone behind the switch-off: the association's two stages and nothing else
    ses.assoc_set(0.0)
    switch_noise(ses, kw["noise"])
    c0 = counters(e)
    hand_over(e, 0, kw)
    ses.step(0, SC.DP, True)
    assert advance(e, c0) == expected(dict(noise=kw["noise"]), 1)
    ses.close()
    e.close()


def test_host_program_with_every_option(orc, tmp_path):
    """slam_pf_main on the generated parity dataset with every option of the associating frame at once: accepted, exit 0, a
    landmark file; twice: the same bytes; without --merge: at least as many landmarks."""
    info = json.loads((GOLDEN / "datasets.json").read_text())["parity"]
    csv = tmp_path / "parity.csv"
    orc.run_tool("gen_dataset", csv, *info["gen_args"])
    exe = PKG_DIR / "lib" / "slam_pf_main"
    merge = ["--merge", "40"]
    rest = ["--landmarks", "32", "--assoc", "9.21", "50", "--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0", "--pole-radius", "0.1",
            "--range-noise", "0.0004", "0.0002", "0.0004", "--prune", "1", "1", "3", "10", "--prune-sight", "128", "0.3", "--prune-fov", "0.1",
            "--refine", "2", "--ess", "0.5"]
    outs = {}
    for run, extra in (("a", merge), ("b", merge), ("no merge", [])):
        lm, mp = tmp_path / f"landmarks_{run}.csv", tmp_path / f"map_{run}.csv"
        r = subprocess.run([str(exe), str(csv), "120", "1079", str(mp), "256", "3"] + rest + extra + ["--landmarks-out", str(lm)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout.count("pose =") == 119
        outs[run] = (r.stdout, lm.read_bytes(), mp.read_bytes())
    assert outs["a"] == outs["b"]
    rows = [[float(v) for v in ln.split(",")] for ln in outs["a"][1].decode().splitlines()]
    assert len(rows) <= 32 and all(len(v) == 2 and np.isfinite(v).all() for v in rows)
    assert len(outs["no merge"][1].decode().splitlines()) >= len(rows)
