"""The specification of the misses of localisation in a known landmark map ("Localisation in a known map";
include/slam_hip.h: slam_localise_miss_dev, slam_localise_detcov_miss_dev, slam_pf_known_map_miss_set) in numpy float32.  TEST
INFRASTRUCTURE shared by test_localise_miss_spec_cpu.py, test_localise_miss_behaviour_cpu.py and the GPU tests.  It imports the
existing specifications and adds NO arithmetic and no second copy of the visibility predicate.

Localisation weighs a particle by its matched pairs and by a clutter term per unmatched detection.  Here it also asks what the
map says the particle SHOULD have seen.  For the known map M [5][L], the poses and the table `localise` (either noise form) made,
with the definitions of _fov_spec.evidence:

  due      = seen & ~hit_now & (r2 <= view_range^2)
  outside  = due & ~in_view            the arc (lo, hi) of the diamond angle; _fov_spec.ALL: nothing is outside
  spared   = due & in_view & hidden    the sight table T of the frame's scan and a margin; T None: nothing is hidden
  missed   = due & in_view & ~hidden

They are read off _fov_spec.evidence run on M broadcast to every particle with every evidence byte at 255 and hit = miss = 1,
cmax = 255: a byte the stage lowered is a miss (_assoc_weight_spec.missed_of; 255 pays any miss, so nothing is pruned).  The
log-likelihood is then _assoc_weight_spec.add(ll, stats, missed, 0, log_clutter, log_miss), left out only when both are 0.
"""
import numpy as np

import _assoc_weight_spec as W
import _fov_spec as V
import _localise_detcov_spec as LD
import _localise_spec as LS
import _sight_spec as S

F = np.float32
ALL = V.ALL


def counts(M, x, y, th, assoc, K, view_range, lo=ALL[0], hi=ALL[1], T=None, margin=None):
    """-> (missed, spared, outside) int32 [n] each; assoc: the table uint8 [n][>= L] of the frame's localise stage."""
    M = np.ascontiguousarray(M, np.float32)
    n, L = len(x), M.shape[1]
    mp = np.broadcast_to(M, (n,) + M.shape)
    ev_in = np.full((n, L), 255, np.uint8)
    mp_out, ev_out, _, spared, outside = V.evidence(mp, x, y, th, None, assoc, K, ev_in, 1, 1, 255, view_range, lo, hi, T, margin)
    missed = W.missed_of(ev_in, None, ev_out, mp, mp_out)
    return missed, spared, outside


def localise(M, x, y, th, zx, zy, noise, gate, log_clutter, log_miss=0.0, view=None, T=None):
    """noise: a meas_var (float: _localise_spec.localise) or (qxx, qxy, qyy) (_localise_detcov_spec.localise).  view: None — the mode
    is off, exactly that function — or (view_range, (lo, hi) or None, margin or None: no line of sight); T: the sight table of the
    frame's scan where a margin is given.
    -> (assoc, stats, ll, missed, spared, outside); the counts None with the mode off."""
    detcov = isinstance(noise, (tuple, list))
    loc = LD.localise if detcov else LS.localise
    if view is None:
        return loc(M, x, y, th, zx, zy, noise, gate, log_clutter) + (None, None, None)
    _, log_clutter, log_miss = W.check_constants(0.0, log_clutter, log_miss)
    view_range, arc, margin = view
    lo, hi = ALL if arc is None else arc
    assoc, stats, ll = loc(M, x, y, th, zx, zy, noise, gate, 0.0)
    missed, spared, outside = counts(M, x, y, th, assoc, len(zx), view_range, lo, hi, T if margin is not None else None, margin)
    if log_clutter != 0 or log_miss != 0:
        ll, _ = W.add(ll, stats, missed, 0.0, log_clutter, log_miss)
    return assoc, stats, ll, missed, spared, outside


def frame_loop(world, n, frames, *, seed, sigma, score_gain, dp, detections, known_map, gate, log_clutter, meas_var=None, miss=None,
               ess=0.0, refine=None, score=True, scans=None):
    """_localise_spec.frame_loop (meas_var given; detections(f) -> (zx, zy)) or _localise_detcov_spec.frame_loop (meas_var None;
    detections(f) -> (zx, zy, (qxx, qxy, qyy))) with `localise` above in place of theirs — what a session does once
    slam_pf_known_map_miss_set was called.  miss: None (off: exactly those loops), or (log_miss, view_range, arc, sight) with arc =
    (lo, hi) or None and sight = (bins, margin) or None, or a function of the frame number that returns either; with sight the table
    is _sight_spec.table of the frame's scan.  Those loops have no seam between their stage and their weights, so the body is
    COPIED here, every stage a call into the specification it came from; test_localise_miss_spec_cpu.py pins the copy to both
    with the mode off.  -> one dict per frame as theirs, plus missed / spared / outside (None where the mode did not run) and
    table."""
    import oracle
    import _refine_spec as R

    x, y, th = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled, out = None, None, True, []
    for f in range(frames):
        bx, by = scans[f] if scans is not None else (world.get("bx"), world.get("by"))
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, dp(f) if callable(dp) else dp, sigma, seed, f)
        if not score:
            sc = np.zeros(n, np.float32)
        elif refine:
            x, y, th, sc, _ = R.refine(oracle, world["meta"], world["edt"], bx, by, x, y, th, *refine)
        else:
            sc, _ = oracle.score_poses_det(world["meta"], world["edt"], bx, by, x, y, th)
        M = known_map(f) if callable(known_map) else known_map
        ms = miss(f) if callable(miss) else miss
        det = detections(f)
        assoc = stats = ll = missed = spared = outside = T = None
        if M is not None and det is not None:
            noise = meas_var if meas_var is not None else det[2]
            view = None
            if ms is not None:
                log_miss, view_range, arc, sight = ms
                T = S.table(bx, by, sight[0]) if sight else None
                view = (view_range, arc, sight[1] if sight else None)
            assoc, stats, ll, missed, spared, outside = localise(M, x, y, th, det[0], det[1], noise, gate, log_clutter,
                                                                 ms[0] if ms is not None else 0.0, view, T)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), logw=logw, anc=anc, resampled=prev_resampled, assoc=assoc,
                        stats=stats, ll=ll, missed=missed, spared=spared, outside=outside, table=T))
    return out
