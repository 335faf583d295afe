"""A session that localises in a known map with EVERY switch against the composed loop of tests/_known_pipeline_spec.py, over the
twelve frames of tests/_known_pipeline_scenes.py, bit for bit and frame by frame: poses, log-weights, ancestors, the stage's stats,
missed / spared / outside, the sight table, the detections the engine holds and their covariances, the gate's verdicts and
frames_resampled, the counts of every reseed and the population behind it, and mean, spread and best after every step and every
reseed — eight combinations of noise form, detector form, miss view, refinement, resample gate and reseed schedule, the last two
with the switches changed mid-run and with the map switched off and everything given again; the launch counters of every
known-map stage after every call; refused calls against a loop that never saw them; and slam_pf_main with every option at once.

The SAME driver (_known_pipeline_spec.drive) makes the calls on the specification's Session and, through `Device` below, on the
package's: the two event lists are compared one by one.  (A known-map session keeps no association table: the stage's stats and
counts, and the log-weights made from its log-likelihoods, stand for it.)"""
import subprocess

import numpy as np
import pytest
import torch

import _known_pipeline_scenes as KS
import _known_pipeline_spec as KP
import test_gpu_spread_session as TS
from __graft_entry__ import PKG_DIR, load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, FRAMES = KS.N, KS.FRAMES
F = np.float32
NOT_READY, INVALID_ARG = -4, -2
FOV = (KS.ARC[0], KS.ARC[1], KS.EDGE)


@pytest.fixture(scope="module")
def world(orc):
    w = KS.make_world()
    return dict(w, d_edt=torch.from_numpy(w["edt"]).to(DEV))


def library_arc():
    """The arc's bounds as the session makes them: float32 sums, then slam_fov_bound — the spec's from here on."""
    pkg = load_package()
    arc = pkg.fov_bound(float(F(FOV[0]) + F(FOV[2]))), pkg.fov_bound(float(F(FOV[1]) - F(FOV[2])))
    assert all(abs(float(a) - float(b)) < 1e-6 for a, b in zip(arc, KS.bounds()))
    return arc


def host(a):
    return torch.as_tensor(a, device=DEV).cpu().numpy()


class Device:
    """The package's session behind the methods of _known_pipeline_spec.Session."""

    def __init__(self, world, ess=0.0, refine=None):
        self.pkg = pkg = load_package()
        m = world["meta"]
        self.e = e = pkg.Engine(0)
        e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
        self.ses = pkg.PfSession(e, N, 0, resample_ess_frac=ess, **KS.KW)
        if refine:
            self.ses.refine_set(*refine)
        self.ses.set_poses(world["x"], world["y"], world["th"])
        self.ess, self.miss, self.on, self.c0 = ess, None, False, self.counters()

    def close(self):
        self.ses.close()
        self.e.close()

    def counters(self):
        e = self.e
        return dict(prepare=e.localise_counts()[0], iso=e.localise_counts()[1], detcov=e.localise_detcov_count(), miss=e.localise_miss_count(),
                    weight=e.assoc_weight_count(), sight=e.sight_counts()[0], detect=e.detect_count(), fit=e.detect_fit_count(),
                    model=e.detect_noise_count(), single=e.pose_reseed_count(), pairs=e.pose_reseed_pairs_count(),
                    other=(e.assoc_counts(), e.assoc_aniso_counts(), e.assoc_detcov_counts(), e.evidence_counts(), e.fov_counts(), e.merge_count(),
                           e.sight_counts()[1], e.frame_fusion_count()))

    def moved(self):
        c1 = self.counters()
        assert c1["other"] == self.c0["other"], "a stage of the mapping side ran"
        d = {k: c1[k] - self.c0[k] for k in c1 if k != "other"}
        self.c0 = c1
        return d

    def refused(self, call, status, error):
        c0 = self.counters()
        with pytest.raises(self.pkg.SlamError) as err:
            call()
        assert err.value.status == status and self.counters() == c0   # (a refused call launches nothing)
        raise error(str(err.value))

    def known_map_set(self, M, form=None, gate=None, log_clutter=None):
        self.on = M is not None
        if M is None:
            return self.ses.known_map_set(None)
        (self.ses.known_map_detcov_set if form == "detcov" else self.ses.known_map_set)(M, gate, log_clutter)
        v = self.ses.known_map_view()
        assert v["nlandmarks"] == M.shape[1] and (v["prepared"] is None) == (form == "detcov")

    def miss_set(self, miss):
        if miss is None:
            self.miss = None
            return self.ses.known_map_miss_set(0.0, 0.0)
        log_miss, view_range, fov, sight = miss
        call = lambda: self.ses.known_map_miss_set(log_miss, view_range, FOV if fov else None, sight)
        try:
            call()
        except self.pkg.SlamError:
            self.refused(call, INVALID_ARG, KP.InvalidArg)
        self.miss = miss

    def detect_set(self, d):
        if d is None:
            return self.ses.detect_set(None)
        call = lambda: self.ses.detect_noise_set(d.get("noise"), d.get("fit"), **d["params"])
        try:
            call()
        except self.pkg.SlamError:
            self.refused(call, INVALID_ARG, KP.InvalidArg)

    def upload(self, det):
        self.e.detections_upload(det[0], det[1])
        if len(det) == 3:
            self.e.detections_cov_upload(*det[2])

    def scan_set(self, bx, by):
        self.e.scan_upload(bx, by)

    def step(self, dp, observing):
        call = lambda: self.ses.step(0, dp, bool(observing))
        before = self.ses.poses()
        try:
            call()
        except self.pkg.SlamError:
            try:
                self.refused(call, NOT_READY, KP.NotReady)
            finally:
                assert np.array_equal(bits(self.ses.poses()), bits(before))
        v = self.ses.device_view()
        self.e.sync()
        rec = dict(pose=self.ses.poses(), logw=host(v["logw"]), anc=host(v["anc"]), det=self.held())
        try:
            rec["stats"] = host(self.ses.known_map_view()["stats"])
        except self.pkg.SlamError:
            rec["stats"] = None   # (no known map was ever set)
        if self.miss is not None:
            rec.update({k: host(a) for k, a in self.ses.known_map_miss_view().items()})
            if self.miss[3] and self.on and observing:   # (a new scan takes the old table with it: only a frame that ran the stage has one)
                rec["table"] = self.e.sight_table()
        return rec

    def held(self):
        try:
            det = self.e.detections()
        except self.pkg.SlamError:
            return None
        try:
            return det + (self.e.detections_cov(),)
        except self.pkg.SlamError:
            return det + (None,)

    def reseed(self, call):
        go = (lambda: self.ses.known_map_reseed(call[1])) if call[0] == "single" else (lambda: self.ses.known_map_reseed_pairs(*call[1:]))
        try:
            return go()
        except self.pkg.SlamError:
            self.refused(go, NOT_READY, KP.NotReady)

    def pending(self):
        return self.ses.device_view()["anc"] is not None

    def population(self):
        return self.ses.poses()

    def reads(self, ref):
        try:
            best = self.ses.best()
        except self.pkg.SlamError as err:
            assert err.status == NOT_READY and "reseeded" in str(err)
            best = None
        verdict = bool(self.e.resample_happened()) if self.ess and self.pending() else None
        return dict(mean=self.ses.mean(ref), spread=self.ses.spread(ref), best=best, verdict=verdict, frames_resampled=self.ses.frames_resampled())


def same(a, b):
    return np.array_equal(bits(np.asarray(a, F)), bits(np.asarray(b, F)))


def compare_reads(g, w, label):
    assert same(g["mean"], w["mean"]), f"{label}: mean"
    assert all(same(a, b) for a, b in zip(g["spread"], w["spread"])), f"{label}: spread"
    assert same(g["spread"][0], g["mean"]), f"{label}: spread's pose is the mean"
    if w["best"] is None:
        assert g["best"] is None, f"{label}: best was not refused"
    else:
        assert g["best"] is not None and g["best"][2] == w["best"][2], f"{label}: best index"
        assert "best_logw" not in w or w["best"][2] == int(np.argmax(w["best_logw"])), f"{label}: best is the argmax of the spec's log-weights"
        assert same(g["best"][0], w["best"][0]) and same(g["best"][1], w["best"][1]), f"{label}: best pose and log-weight"
    assert g["verdict"] == w["verdict"], f"{label}: the gate's verdict"
    assert g["frames_resampled"] == w["frames_resampled"], f"{label}: frames_resampled"


def compare_frame(g, w, label):
    assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label}: log-weights"
    assert np.array_equal(g["anc"], w["anc"]), f"{label}: ancestors"
    assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label}: poses"
    for k in ("stats", "missed", "spared", "outside"):
        if w[k] is not None:
            assert np.array_equal(g[k], w[k]), f"{label}: {k}"
    if w["table"] is not None:
        assert "table" in g and same(g["table"], w["table"]), f"{label}: sight table"
    if w["det"] is None:
        assert g["det"] is None, f"{label}: detections"
    else:
        assert g["det"] is not None and same(g["det"][0], w["det"][0]) and same(g["det"][1], w["det"][1]), f"{label}: detections"
        assert (g["det"][2] is None) == (w["det"][2] is None), f"{label}: the detections carry covariances"
        if w["det"][2] is not None:
            assert all(same(a, b) for a, b in zip(g["det"][2], w["det"][2])), f"{label}: the detections' covariances"


def compare_events(got, want, name):
    assert [e[:2] for e in got] == [e[:2] for e in want], f"{name}: the calls"
    for g, w in zip(got, want):
        label = f"{name}: {w[0]} {w[1]}"
        if w[0] == "refused":
            assert g[2:] == w[2:], label
        elif w[0] == "frame":
            compare_frame(g[2], w[2], label)
            compare_reads(g[3], dict(w[3], best_logw=w[2]["logw"]), label)
            assert g[4] == w[4], f"{label}: launches {g[4]} != {w[4]}"
        else:
            label += f" {w[2]}"
            assert tuple(g[3]) == tuple(w[3]), f"{label}: counts {g[3]} != {w[3]}"
            assert g[6] == w[6], f"{label}: pending gather"
            assert np.array_equal(bits(g[4]), bits(w[4])), f"{label}: the population behind the call"
            compare_reads(g[5], w[5], label)
            assert g[7] == w[7], f"{label}: launches {g[7]} != {w[7]}"


def events(ses, kw, frames=FRAMES):
    kw = {k: v for k, v in kw.items() if k not in ("refine", "ess")}
    return KP.drive(ses, KS.SCANS, frames, dp=KS.DP, gate=KS.GATE, log_clutter=KS.CLUTTER, **kw)


def spec_events(world, kw, arc, frames=FRAMES):
    ses = KP.Session(world, N, ess=kw.get("ess", 0.0), refine=kw.get("refine"), arc=tuple(arc), **KS.KW)
    return events(ses, kw, frames)


@pytest.mark.parametrize("name", list(KS.COMBOS))
def test_session_equals_the_composed_loop(world, name):
    arc = library_arc()
    KS.check_not_vacuous(world, name, arc)
    kw = KS.schedule(name)
    want = spec_events(world, kw, arc)
    dev = Device(world, ess=kw.get("ess", 0.0), refine=kw.get("refine"))
    got = events(dev, kw)
    compare_events(got, want, name)
    dev.close()


def test_launch_counters_follow_the_schedule(world):
    """Every known-map stage, on or off, by the engine's counters over the switching run: after every step and every reseed call
    what moved is what the schedule says (compare_events: `launches`), a no-op reseed and a refused frame move none (Device.refused),
    and over the whole run the totals are those the schedule adds up to."""
    arc = library_arc()
    kw = KS.schedule("everything, switching")
    want = spec_events(world, kw, arc)
    dev = Device(world, ess=kw["ess"], refine=kw["refine"])
    c0 = dev.counters()
    got = events(dev, kw)
    c1 = dev.counters()
    moved = [e[4] if e[0] == "frame" else e[7] for e in got if e[0] != "refused"]
    assert moved == [e[4] if e[0] == "frame" else e[7] for e in want if e[0] != "refused"]
    total = {k: sum(m[k] for m in moved) for k in moved[0]}
    assert {k: c1[k] - c0[k] for k in total} == total
    # iso 3 .. 5 (frame 5 does not observe): two prepares (the form, then the larger map), the misses on from frame 2, line of sight from 7
    assert total == dict(prepare=2, iso=0, detcov=2, miss=9, weight=11, sight=5, detect=11, fit=11, model=9, single=4, pairs=3)
    noop = [e for e in got if e[0] == "reseed" and e[6]]
    assert len(noop) == 1 and noop[0][1] == KS.LONE and not any(noop[0][7].values())
    dev.close()


@pytest.mark.parametrize("name", ["everything, switching", "everything, restart"])
def test_refused_calls_leave_the_session_as_it_was(world, name):
    """The device is asked what is refused — the detector's model under the isotropic form, the frame whose detector lost its
    model, a reseed and the misses while the mode is off — and the specification is NOT: its host gives the model again in front
    of the frame.  Everything accepted is the same."""
    arc = library_arc()
    kw = KS.schedule(name)
    frames = 9
    never = dict(kw, tries=None, regive=(), redetect=kw.get("regive", ()))
    want = spec_events(world, never, arc, frames)
    dev = Device(world, ess=kw["ess"], refine=kw["refine"])
    got = events(dev, kw, frames)
    refused = [e for e in got if e[0] == "refused"]
    assert len(refused) == 2
    compare_events([e for e in got if e[0] != "refused"], want, name)
    dev.close()


def test_host_program_with_every_known_map_option(orc, tmp_path):
    """slam_pf_main on the moving-sensor scene with every known-map option at once — the map of the scene's poles, the detector
    with fit and noise model, the misses with arc and line of sight, pair reseeds every second frame, refinement, the resample
    gate, --spread-out — in a process of its own under a time limit: its pose log with the four counts and every line of its
    spread file are those of a session driven from Python through the same calls (the session the tests above pin to the composed
    loop); twice: the same bytes; the counts add up to the population or to nothing."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv = tmp_path / "scene.csv"
    TS.write_scene(csv)
    lines = csv.read_text().splitlines()
    km = tmp_path / "known.csv"
    km.write_text("".join(f"{x:f},{y:f}\n" for x, y in KS.MAP_A[:2].T))
    n, seed, every = 256, 3, 2
    gate, map_var, clutter = 9.21, 0.05, -2.5
    noise, radius = (0.0025, 0.00015625, 0.0025), 0.1
    opts = ["--known-map", str(km), f"{gate}", f"{map_var}", f"{clutter}", "--detect", "--pole-radius", f"{radius}", "--range-noise", *(f"{v}" for v in noise),
            "--known-miss", f"{KS.LOG_MISS}", f"{KS.VIEW_RANGE}", "--known-miss-fov", f"{KS.EDGE}", "--known-miss-sight", "128", "0.3",
            "--known-reseed-pairs", "0.25", f"{KS.TOL}", f"{KS.MIN_SEP}", f"{every}", "--refine", "1", "--ess", "0.5"]

    def run(tag):
        r = subprocess.run([str(exe), str(csv), str(len(lines)), str(len(lines[0].split(","))), str(tmp_path / f"map_{tag}.csv"), str(n), str(seed)]
                           + opts + ["--spread-out", str(tmp_path / f"spread_{tag}.csv")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout, (tmp_path / f"spread_{tag}.csv").read_text()

    out = run("a")
    assert run("b") == out
    tails = [[int(v) for v in ln.split("reseed-pairs = ")[1].split()] for ln in out[0].splitlines() if ln.startswith("pose =")]
    assert len(tails) == len(lines) - 1 and all(sum(t) == 0 for t in tails[0::2]) and all(0 < sum(t) <= n for t in tails[1::2])
    assert any(t[0] > 0 for t in tails)

    M = np.zeros((5, KS.MAP_A.shape[1]), F)
    M[0], M[1] = [[float(f"{v:f}") for v in row] for row in KS.MAP_A[:2]]
    M[2] = M[4] = map_var

    def configure(pkg, e, ses, ang):
        ses.refine_set(0.025, 0.004363, 1)
        ses.known_map_detcov_set(M, gate, clutter)
        ses.detect_noise_set(noise, pkg.DetectFit.default(radius=radius))
        ses.known_map_miss_set(KS.LOG_MISS, KS.VIEW_RANGE, (float(ang[0]), float(ang[-1]), KS.EDGE), (128, 0.3))

    calls = [0]

    def after(ses):
        calls[0] += 1
        c = ses.known_map_reseed_pairs(0.25, KS.TOL, KS.MIN_SEP) if calls[0] % every == 0 else (0, 0, 0, 0)
        return "  reseed-pairs = %d %d %d %d" % c

    log, want, _ = TS.python_run(orc, csv, 0.5, n=n, seed=seed, meas_var=0.01, configure=configure, observe=True, after=after)
    assert log == out[0]
    got = TS.parse(tmp_path / "spread_a.csv")
    assert [g[0] for g in got] == [w[0] for w in want] == list(range(2, len(lines) + 1))
    for g, w in zip(got, want):
        assert np.array_equal(bits(g[1]), bits(w[1])) and np.array_equal(bits(g[2]), bits(w[2])), (g, w)
