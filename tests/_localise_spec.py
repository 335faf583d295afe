"""The specification of localisation in a known landmark map ("Localisation in a known map";
include/slam_hip.h: slam_known_map_prepare_dev, slam_localise_dev, slam_pf_known_map_set) in numpy float32.  TEST INFRASTRUCTURE
shared by test_localise_spec_cpu.py, test_localise_behaviour_cpu.py and the GPU tests.  It imports the existing specifications
and adds NO arithmetic: the stage is the association with create = 0 and the update's log-likelihood on ONE map every particle
shares, plus the clutter term of the unexplained; the map the update returns is thrown away.

The known map is M float32 [5][L]: planes mx, my, P_xx, P_xy, P_yy as in a row; a slot with P_xx < 0 holds no landmark.
"""
import numpy as np

import _assoc_spec as A
import _assoc_weight_spec as W

F = np.float32
NONE = A.NONE


def localise(M, x, y, th, zx, zy, meas_var, gate, log_clutter):
    """-> (assoc uint8 [n][L], stats int32 [n][3] = matched, 0, K - matched, ll float32 [n]).  gate finite and > 0;
    log_clutter finite and <= 0 (0: the clutter step is left out)."""
    M = np.ascontiguousarray(M, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    n = len(x)
    (log_clutter,) = W.check_constants(0.0, log_clutter, 0.0)[1:2]
    mp = np.broadcast_to(M, (n,) + M.shape)
    assoc, stats = A.associate(mp, x, y, th, None, zx, zy, meas_var, gate, gate, 0)
    _, ll = A.update(mp, x, y, th, None, assoc, zx, zy, meas_var)   # the map it returns is thrown away
    if log_clutter != 0:
        ll, _ = W.add(ll, stats, None, 0.0, log_clutter, 0.0)
    return assoc, stats, ll


def frame_loop(world, n, frames, *, seed, sigma, meas_var, score_gain, dp, detections, known_map, gate, log_clutter, ess=0.0,
               refine=None, score=True, scans=None):
    """_assoc_spec.frame_loop with its associate / update pair replaced by `localise` on the fixed known_map; no map is carried.
    Motion, score or refine, weights (logweight_carry), the ESS gate and the resample are unchanged.  known_map: M, or a function
    of the frame number that returns M or None (None: the mode is off in that frame); detections(f) -> (zx, zy), or None: a frame
    with use_observations = 0 — both are today's frame, plain weights.  scans: optional per-frame (bx, by) for the scorer.
    -> one dict per frame: pose [3][n] with the frame's resample applied, logw, anc, resampled, and assoc / stats / ll indexed like
    logw (None where the stage did not run)."""
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
        det = detections(f)
        assoc = stats = ll = None
        if M is not None and det is not None:
            assoc, stats, ll = localise(M, x, y, th, det[0], det[1], meas_var, gate, log_clutter)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), logw=logw, anc=anc, resampled=prev_resampled, assoc=assoc,
                        stats=stats, ll=ll))
    return out
