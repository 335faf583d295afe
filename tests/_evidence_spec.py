"""The specification of landmark existence evidence ("Existence evidence"; include/slam_hip.h:
slam_landmark_evidence_dev, slam_evidence_init_dev, slam_pf_prune_set) in numpy integers and float32, one rounded operation per
line.  TEST INFRASTRUCTURE shared by test_evidence_spec_cpu.py, test_evidence_behaviour_cpu.py and the GPU tests.  It reuses
tests/_assoc_spec.py for the association and the update, and nothing of the package.

Every particle keeps one evidence byte c in [0, cmax] per landmark slot beside its row.  Behind the update of a frame a landmark
that took a detection gains `hit`, one that lies within view_range of the particle's pose and took none loses `miss`, and one that
cannot pay the miss is PRUNED: its slot gets the bits of a slot that was never used, so the association hands it out again.
"""
import numpy as np

import _assoc_spec as A

F = np.float32
FRESH = (F(0.0), F(0.0), F(-1.0), F(0.0), F(0.0))   # the five planes of a slot that was never used


def evidence_init(map_rows, value, L=None, ev_stride=None):
    """c = seen ? value : 0 over every row of map_rows [rows][5][plane_stride]; padding columns 0 -> uint8 [rows][ev_stride]."""
    map_rows = np.ascontiguousarray(map_rows, np.float32)
    L = map_rows.shape[2] if L is None else L
    stride = L if ev_stride is None else ev_stride
    assert 0 <= value <= 255 and stride >= L
    ev = np.zeros((map_rows.shape[0], stride), np.uint8)
    seen = ~(map_rows[:, 2, :L] < 0)
    ev[:, :L] = np.where(seen, np.uint8(value), np.uint8(0))
    return ev


def evidence(map_rows, x, y, anc, assoc, K, ev_in, hit, miss, cmax, view_range, L=None, in_place=False):
    """map_rows: float32 [n][5][plane_stride], the rows AFTER the frame's update; x, y: the poses the update used; assoc: uint8
    [n][>= L] the frame's table; K: the number of detections of the frame; ev_in: uint8 [rows][ev_stride]; particle i reads evidence
    row anc[i] (anc None: i).  in_place (anc must be None): the padding columns of the evidence are left alone, else they are 0.
    -> (map_out, ev_out uint8 [n][ev_stride], stats int32 [n][2] = pruned, seen after pruning)."""
    assert not (in_place and anc is not None)
    map_rows = np.ascontiguousarray(map_rows, np.float32)
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    ev_in = np.ascontiguousarray(ev_in, np.uint8)
    n = len(x)
    L = map_rows.shape[2] if L is None else L
    stride = ev_in.shape[1]
    for v in (hit, miss, cmax):
        assert 1 <= int(v) <= 255
    assert np.isfinite(view_range) and view_range > 0 and stride >= L and 0 <= K <= A.MAX_DETECTIONS
    hit, miss, cmax = int(hit), int(miss), int(cmax)
    with np.errstate(all="ignore"):
        range2 = F(view_range) * F(view_range)   # rounded once; a large range gives inf: every finite mean is visible
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    c = ev_in[src][:, :L].astype(np.int64)
    a = np.asarray(assoc)[:n, :L].astype(np.int64)
    mx, my, pxx = map_rows[:n, 0, :L], map_rows[:n, 1, :L], map_rows[:n, 2, :L]
    px, py = x[:, None], y[:, None]
    seen = ~(pxx < 0)
    hit_now = a < K
    with np.errstate(all="ignore"):
        dx = mx - px
        dy = my - py
        t = dx * dx
        u = dy * dy
        r2 = t + u
        visible = r2 <= range2
    miss_now = seen & ~hit_now & visible
    prune = miss_now & (c < miss)
    out = np.where(seen & hit_now, np.minimum(c + hit, cmax), c)
    out = np.where(miss_now & ~prune, c - miss, out)
    out = np.where(prune | ~seen, 0, out)
    map_out = map_rows.copy()
    for p in range(5):
        map_out[:n, p, :L] = np.where(prune, FRESH[p], map_rows[:n, p, :L])
    ev_out = ev_in[src].copy() if in_place else np.zeros((n, stride), np.uint8)
    ev_out[:, :L] = out.astype(np.uint8)
    stats = np.stack([prune.sum(axis=1), (seen & ~prune).sum(axis=1)], axis=1).astype(np.int32)
    return map_out, ev_out, stats


def frame_loop(world, n, frames, *, seed, sigma, meas_var, score_gain, dp, detections, gate, new_gate, create, prune, ess=0.0,
               refine=None, score=True, ev0=None):
    """_assoc_spec.frame_loop with the evidence stage between the update and the weights: what a rows session does once
    slam_pf_assoc_set and slam_pf_prune_set were called.  prune: (hit, miss, cmax, view_range), or None (pruning off: then exactly
    _assoc_spec.frame_loop), or a function of the frame number that returns either.  detections(f) -> (zx, zy), or None: a frame
    without a detection hand-over (slam_pf_step without observations) — maps and evidence only follow their ancestors.  Switching
    pruning on (frame 0, or behind a frame that ran without) initialises the evidence from the maps with value = cmax (ev0: the
    evidence to start from instead).
    -> one dict per frame as _assoc_spec.frame_loop's, plus ev [n][L] with the frame's resample applied (what
    slam_pf_get_evidence_host returns), ev_raw (indexed like logw: the device view) and ev_stats (None on a frame without the stage)."""
    import oracle
    import _refine_spec as R

    x, y, th, mp = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th", "mp"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled, out = None, None, True, []
    ev, was_on = ev0, False
    for f in range(frames):
        pr = prune(f) if callable(prune) else prune
        if pr and not was_on and (ev is None or f > 0):
            ev = evidence_init(mp, pr[2])   # switched on: a map that is there is trusted (indexed like mp: before the pending gather)
        was_on = bool(pr)
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, dp(f) if callable(dp) else dp, sigma, seed, f)
        if not score:
            sc = np.zeros(n, np.float32)
        elif refine:
            x, y, th, sc, _ = R.refine(oracle, world["meta"], world["edt"], world["bx"], world["by"], x, y, th, *refine)
        else:
            sc, _ = oracle.score_poses_det(world["meta"], world["edt"], world["bx"], world["by"], x, y, th)
        det = detections(f)
        assoc = stats = ev_stats = None
        if det is None:   # no hand-over: maps and evidence follow their particles, the weights are the score's
            if anc is not None:
                mp = mp[anc]
                ev = ev[anc] if pr else ev
            ll = None
        else:
            zx, zy = det
            assoc, stats = A.associate(mp, x, y, th, anc, zx, zy, meas_var, gate, new_gate, create)
            mp, ll = A.update(mp, x, y, th, anc, assoc, zx, zy, meas_var)
            if pr:
                mp, ev, ev_stats = evidence(mp, x, y, anc, assoc, len(zx), ev, *pr)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled,
                        assoc=assoc, stats=stats, ev=ev[anc] if pr else None, ev_raw=ev if pr else None, ev_stats=ev_stats))
    return out
