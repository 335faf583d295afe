"""The specification of localisation in a known landmark map under a measurement covariance PER DETECTION (DESIGN.md section 7,
"Localisation in a known map"; include/slam_hip.h: slam_localise_detcov_dev, slam_pf_known_map_detcov_set) in numpy float32.  TEST
INFRASTRUCTURE shared by test_localise_detcov_spec_cpu.py, test_localise_detcov_behaviour_cpu.py and the GPU tests.  It is
tests/_localise_spec.py with the pair of tests/_assoc_detcov_spec.py in the place of the isotropic pair and adds NO arithmetic: the
association with create = 0 and the update's log-likelihood under S = P + R_w(theta_i, k) on ONE map every particle shares, plus
the clutter term of the unexplained; the map the update returns is thrown away.

The known map is M float32 [5][L] as in _localise_spec.py; Q_k = (qxx[k], qxy[k], qyy[k]) as in _assoc_detcov_spec.py.
"""
import numpy as np

import _assoc_detcov_spec as AD
import _assoc_weight_spec as W

F = np.float32
NONE = AD.NONE


def localise(M, x, y, th, zx, zy, meas_covs, gate, log_clutter):
    """-> (assoc uint8 [n][L], stats int32 [n][3] = matched, 0, K - matched, ll float32 [n]).  gate finite and > 0;
    log_clutter finite and <= 0 (0: the clutter step is left out)."""
    M = np.ascontiguousarray(M, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    n = len(x)
    (log_clutter,) = W.check_constants(0.0, log_clutter, 0.0)[1:2]
    mp = np.broadcast_to(M, (n,) + M.shape)
    assoc, stats = AD.associate(mp, x, y, th, None, zx, zy, meas_covs, gate, gate, 0)
    _, ll = AD.update(mp, x, y, th, None, assoc, zx, zy, meas_covs)   # the map it returns is thrown away
    if log_clutter != 0:
        ll, _ = W.add(ll, stats, None, 0.0, log_clutter, 0.0)
    return assoc, stats, ll


def frame_loop(world, n, frames, *, seed, sigma, score_gain, dp, detections, known_map, gate, log_clutter, ess=0.0, refine=None,
               score=True, scans=None):
    """_localise_spec.frame_loop with `localise` above in place of its own — what a session does once
    slam_pf_known_map_detcov_set was called.  detections(f) -> (zx, zy, (qxx, qxy, qyy)), or None: a frame with
    use_observations = 0.  Everything else as there.  -> one dict per frame as _localise_spec.frame_loop's."""
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
            assoc, stats, ll = localise(M, x, y, th, det[0], det[1], det[2], gate, log_clutter)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), logw=logw, anc=anc, resampled=prev_resampled, assoc=assoc,
                        stats=stats, ll=ll))
    return out
