"""A rows session with data association and pruning (slam_pf_assoc_set + slam_pf_prune_set) against the frame loop of
tests/_evidence_spec.py, frame by frame and bit for bit: poses, map rows, evidence (slam_pf_get_evidence_host and the device
view), stats, log-weights and ancestors — resampling every frame, gated, with a frame without a detection hand-over and one with
K = 0, across slam_pf_set_map_host / slam_pf_reset and the switches; plus the refusals, and a session that never switches pruning
on is the session it is without the feature."""
import numpy as np
import pytest
import torch

import _assoc_spec as A
import _evidence_spec as E
import _shard_worker as W
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES = 300, 40, 8
GATE, NEW_GATE = 9.21, 50.0
PRUNE = (1, 1, 4, 3.5)      # hit, miss, cmax, view_range: the true points lie within ~4.2 m, the false ones within ~8.5 m
GATE_ESS = 0.5
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
DP = [0.01, -0.005, 0.002]
TRUE = np.random.default_rng(3).uniform(-3, 3, (7, 2)).astype(np.float32)


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, bx, by, _ = W.make_world(L=L)
    x, y, th, _ = W.init_state(N, 0, np.zeros((0, 2), np.float32))
    mp = np.zeros((N, 5, L), np.float32)
    mp[:, 2] = -1.0                              # the maps start empty
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), bx=bx, by=by, x=x, y=y, th=th, mp=mp)


def detections(f):
    """A handful of the true points (each missed one frame in four) as the moving sensor sees them, plus two false ones."""
    rng = np.random.default_rng(500 + f)
    keep = rng.random(len(TRUE)) >= 0.25
    z = TRUE[keep] - np.float32(f + 1) * np.array(DP[:2], np.float32) + 0.02 * rng.standard_normal((int(keep.sum()), 2)).astype(np.float32)
    z = np.concatenate([z, rng.uniform(-6, 6, (2, 2)).astype(np.float32)])
    z = z[rng.permutation(len(z))].astype(np.float32)
    return z[:, 0].copy(), z[:, 1].copy()


EMPTY = (np.zeros(0, np.float32), np.zeros(0, np.float32))


def reference(world, frames=FRAMES, ess=0.0, prune=PRUNE, det=detections):
    return E.frame_loop(world, N, frames, dp=DP, detections=det, gate=GATE, new_gate=NEW_GATE, create=1, prune=prune, ess=ess, **KW)


def _engine(world):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    return e


def open_session(world, ess=0.0, layout="rows", comm_group=None, assoc=True):
    pkg = load_package()
    e = _engine(world)
    comm = pkg.Comm.local(e, comm_group, 0) if comm_group else None
    ses = pkg.PfSession(e, N, L, comm=comm, resample_ess_frac=ess, map_layout=layout, **KW)
    if assoc:
        ses.assoc_set(GATE, NEW_GATE, True)
    ses.set_poses(world["x"], world["y"], world["th"])
    ses.set_map(world["mp"])
    return e, ses, comm


def close_session(e, ses, comm):
    ses.close()
    if comm:
        comm.close()
    e.close()


def step(e, ses, f, det=detections, pruning=True):
    """Frame f -> what the reference returns for it."""
    d = det(f)
    if d is None:
        ses.step(0, DP, False)                   # no hand-over
    else:
        e.detections_upload(*d)
        ses.step(0, DP, True)
    v = ses.device_view()
    e.sync()
    fr = dict(pose=ses.poses(), map=ses.maps(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
              anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy())
    if pruning:
        ev = ses.evidence_view()
        fr["ev"] = ses.evidence()
        fr["ev_raw"] = torch.as_tensor(ev["ev"], device=DEV).cpu().numpy()
        fr["ev_stats"] = torch.as_tensor(ev["stats"], device=DEV).cpu().numpy()
    return fr


def compare(g, w, label, pruning=True):
    assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label}: log-weights"
    assert np.array_equal(g["anc"], w["anc"]), f"{label}: ancestors"
    assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label}: poses"
    assert np.array_equal(bits(g["map"]), bits(w["map"])), f"{label}: map rows"
    if pruning:
        assert np.array_equal(g["ev"], w["ev"]), f"{label}: evidence (host)"
        assert np.array_equal(g["ev_raw"][:, :L], w["ev_raw"]) and np.all(g["ev_raw"][:, L:] == 0), f"{label}: evidence (view)"
        if w["ev_stats"] is not None:
            assert np.array_equal(g["ev_stats"], w["ev_stats"]), f"{label}: stats"


def run(world, want, ess=0.0, det=detections, frames=FRAMES):
    e, ses, comm = open_session(world, ess=ess)
    ses.prune_set(*PRUNE)
    c0, a0 = e.evidence_counts(), e.assoc_counts()
    for f in range(frames):
        compare(step(e, ses, f, det), want[f], f"frame {f}")
    counts = tuple(np.subtract(e.evidence_counts(), c0)), tuple(np.subtract(e.assoc_counts(), a0)), ses.frames_resampled()
    close_session(e, ses, comm)
    return counts


def test_resampling_every_frame(world):
    want = reference(world)
    st = np.stack([w["ev_stats"] for w in want])
    assert st[..., 0].sum() > 0 and st[..., 1].max() > 3                        # landmarks pruned, maps grown
    # both visible and invisible seen landmarks occur (the last frame's rows against the poses they belong to)
    last = want[-1]
    r = np.hypot(last["map"][:, 0] - last["pose"][0][:, None], last["map"][:, 1] - last["pose"][1][:, None])[~(last["map"][:, 2] < 0)]
    assert (r <= PRUNE[3]).any() and (r > PRUNE[3]).any()
    ev, assoc, _ = run(world, want)
    assert ev == (FRAMES, 0) and assoc == (FRAMES, FRAMES)


def test_gated_session(world):
    """Kept frames run the stage in place, resampled ones through the gather into the other buffer."""
    want = reference(world, ess=GATE_ESS)
    verdicts = [w["resampled"] for w in want]
    assert True in verdicts[:-1] and False in verdicts[:-1], verdicts
    ev, _, resampled = run(world, want, ess=GATE_ESS)
    assert ev == (FRAMES, 0) and resampled == sum(verdicts[:-1])


def test_frames_without_a_hand_over_and_without_detections(world):
    """Frame 3 carries no hand-over: the evidence only follows its ancestors.  Frame 5 hands over K = 0 detections: an observing
    frame, every visible seen landmark takes a miss."""
    det = lambda f: None if f == 3 else EMPTY if f == 5 else detections(f)
    want = reference(world, det=det)
    assert np.array_equal(want[3]["ev_raw"], want[2]["ev_raw"][want[2]["anc"]]) and want[3]["ev_stats"] is None
    assert want[5]["ev_stats"][:, 0].sum() > 0 and np.all(want[5]["ev_raw"] <= want[4]["ev_raw"][want[4]["anc"]])
    ev, assoc, _ = run(world, want, det=det)
    assert ev == (FRAMES - 1, 0) and assoc == (FRAMES - 1, FRAMES - 1)
    # ... and the same under the gate, where a frame behind a kept one gathers nothing
    want = reference(world, ess=GATE_ESS, det=det)
    run(world, want, ess=GATE_ESS, det=det)


def test_maps_replaced_mid_run(world):
    """slam_pf_reset and slam_pf_set_map_host / _dev while pruning is on: the evidence is made anew, 0 for unseen slots and cmax
    for the slots of a loaded map; the session then runs as a new one from that map."""
    loaded = reference(world, frames=3, prune=None)[-1]["map"].copy()           # a map with seen and unseen slots
    seen = ~(loaded[:, 2] < 0)
    assert seen.any() and not seen.all()
    start = dict(world, mp=loaded)
    want = reference(start, frames=3)
    e, ses, comm = open_session(world)
    ses.prune_set(*PRUNE)
    for f in range(3):
        step(e, ses, f)
    c0 = e.evidence_counts()
    ses.reset([0.0, 0.0, 0.0])
    assert np.all(ses.evidence() == 0) and np.all(ses.maps()[:, 2] == -1.0)
    ses.set_poses(world["x"], world["y"], world["th"])
    ses.set_map(loaded)
    assert np.array_equal(ses.evidence(), np.where(seen, PRUNE[2], 0))
    assert e.evidence_counts() == (c0[0], c0[1] + 2)
    for f in range(3):
        compare(step(e, ses, f), want[f], f"after set_map, frame {f}")
    ses.reset([0.0, 0.0, 0.0])
    d_rows = torch.as_tensor(loaded).to(DEV)
    ses.set_map_dev(d_rows, 5 * L, L)
    assert np.array_equal(ses.evidence(), np.where(seen, PRUNE[2], 0))
    close_session(e, ses, comm)


def test_switching_pruning_off_and_on(world):
    """Off for frames 3 and 4 (the session then runs association alone, not one evidence launch), on again before frame 5: the
    evidence starts again from the maps as they are, with cmax."""
    prune = lambda f: None if f in (3, 4) else PRUNE
    want = reference(world, prune=prune)
    e, ses, comm = open_session(world)
    c0 = e.evidence_counts()
    ses.prune_set(*PRUNE)
    for f in range(FRAMES):
        if f == 3:
            ses.prune_set(0)
            c3 = e.evidence_counts()
        if f == 5:
            assert e.evidence_counts() == c3
            ses.prune_set(*PRUNE)
        compare(step(e, ses, f, pruning=prune(f) is not None), want[f], f"frame {f}", pruning=prune(f) is not None)
    assert tuple(np.subtract(e.evidence_counts(), c0)) == (FRAMES - 2, 2)
    for bad in ((256, 1, 4, 3.5), (1, 0, 4, 3.5), (1, 1, 300, 3.5), (1, 1, 4, 0.0), (1, 1, 4, float("nan")), (1, 1, 4, float("inf")), (-1, 1, 4, 3.5)):
        with pytest.raises(load_package().SlamError) as err:
            ses.prune_set(*bad)
        assert err.value.status == -2, bad
    close_session(e, ses, comm)


def test_association_off_takes_pruning_with_it(world):
    pkg = load_package()
    e, ses, comm = open_session(world)
    ses.prune_set(*PRUNE)
    step(e, ses, 0)
    ses.assoc_set(0.0)
    c0 = e.evidence_counts()
    with pytest.raises(pkg.SlamError) as err:
        ses.prune_set(*PRUNE)
    assert err.value.status == -2 and "data association" in str(err.value)
    e.obs_upload(np.arange(3, dtype=np.int32), TRUE[:3, 0].copy(), TRUE[:3, 1].copy(), L)
    ses.step(0, DP, True)
    ses.assoc_set(GATE, NEW_GATE, True)                                          # association on again: pruning stays off
    step(e, ses, 2, pruning=False)
    e.sync()
    assert e.evidence_counts() == c0
    close_session(e, ses, comm)


def _refused(pkg, ses):
    with pytest.raises(pkg.SlamError) as err:
        ses.prune_set(*PRUNE)
    assert err.value.status == -2 and "data association" in str(err.value), str(err.value)
    for call in (ses.evidence_view, ses.evidence):
        with pytest.raises(pkg.SlamError) as err:
            call()
        assert err.value.status == -4


@pytest.mark.parametrize("case", ["association off", "split", "sharded"])
def test_refusals(world, case):
    """... and the session then steps exactly as one that was never asked."""
    pkg = load_package()
    group = pkg.LocalGroup(1) if case == "sharded" else None
    layout = "split" if case == "split" else "rows"
    ids = np.arange(5, dtype=np.int32)
    out = []
    for ask in (False, True):
        e, ses, comm = open_session(world, layout=layout, comm_group=group if ask else None, assoc=False)
        if ask:
            if case != "association off":
                with pytest.raises(pkg.SlamError):
                    ses.assoc_set(GATE, NEW_GATE, True)
            _refused(pkg, ses)
        frames = []
        for f in range(2):
            e.obs_upload(ids, TRUE[:5, 0].copy(), TRUE[:5, 1].copy(), L)
            ses.step(0, DP, True)
            frames.append((ses.poses(), ses.maps()))
        assert e.evidence_counts() == (0, 0)
        out.append(frames)
        close_session(e, ses, comm)
    if group:
        group.close()
    for f in range(2):
        for g, w in zip(out[1][f], out[0][f]):
            assert np.array_equal(bits(g), bits(w)), f"{case}: frame {f}"


def test_pruning_never_switched_on_is_the_session_as_it_was(world):
    want = A.frame_loop(world, N, FRAMES, dp=DP, detections=detections, gate=GATE, new_gate=NEW_GATE, create=1, **KW)
    for ess, ref in ((0.0, want), (GATE_ESS, A.frame_loop(world, N, FRAMES, dp=DP, detections=detections, gate=GATE, new_gate=NEW_GATE,
                                                           create=1, ess=GATE_ESS, **KW))):
        e, ses, comm = open_session(world, ess=ess)
        a0 = e.assoc_counts()
        for f in range(FRAMES):
            compare(step(e, ses, f, pruning=False), ref[f], f"ess={ess} frame {f}", pruning=False)
        assert e.evidence_counts() == (0, 0) and tuple(np.subtract(e.assoc_counts(), a0)) == (FRAMES, FRAMES)
        with pytest.raises(load_package().SlamError) as err:
            ses.evidence_view()
        assert err.value.status == -4
        close_session(e, ses, comm)
