"""The frame of an associating rows session with EVERY switch, composed from the stage specifications ("The
whole associating frame"; csrc/pf_session_frame.hip: pf_step_impl, update_rows).  TEST INFRASTRUCTURE shared by
test_pipeline_spec_cpu.py and test_gpu_pipeline_session.py.  It adds NO arithmetic: every stage is a function of
tests/_assoc_spec.py, _assoc_aniso_spec.py, _assoc_detcov_spec.py, _evidence_spec.py, _sight_spec.py, _fov_spec.py,
_merge_spec.py, _detect_noise_spec.py (which is _detect_fit_spec.py and _detect_spec.py without a model), _refine_spec.py or of
the oracle, and what is stated here is only the plumbing between them — which stage runs, in which order, on which rows, poses,
table, evidence and scan:

  detections  the detector on the frame's scan when it is on (the uploaded ones are then not read), else the uploaded ones
  motion      from the previous frame's ancestors; then the scan-match score, or the refinement: every later stage reads the
              REFINED poses
  associate   under the noise form in force, on the rows of the previous frame behind its ancestors
  update      under the same form, with the table just made
  evidence    (pruning on) on the rows the update wrote, with the evidence of the previous frame behind the same ancestors:
              with a field of view when that is on (and the sight table of THIS frame's scan when line of sight is on too), else
              with line of sight when that is on, else plain.  Line of sight and field of view without pruning run nothing.
  merge       on the rows AND the evidence the stages above wrote, with the frame's table; without pruning: no evidence
  weights, resample gate, resample

A frame without a detection hand-over (detections(f) is None) runs none of the landmark stages: maps and evidence follow their
ancestors.  Under ("detcov",) an observing frame whose detections carry no covariance — uploaded without, or from a detector
without a noise model — raises NotReady, as the session refuses the frame before its first launch.

The switches between frames.  A noise form given anew (slam_pf_assoc_set, slam_pf_assoc_cov_set, slam_pf_assoc_detcov_set with a
gate > 0) changes the noise form and the gates and NOTHING else: pruning with its evidence bytes, line of sight, field of view,
merging and the detector stay as they were — here: `noise` is a function of the frame and the other arguments do not depend on
it.  A 2x2 Q equal to (meas_var, 0, meas_var) is the isotropic form.  Only slam_pf_assoc_set(0, ..) clears the other switches;
with everything switched on again behind it (`restart`) the frame runs as a fresh session's would from the same poses and maps:
the one thing lost is the evidence, which slam_pf_prune_set initialises from the maps again (cmax where a landmark is seen).
"""
import numpy as np

import _assoc_aniso_spec as AA
import _assoc_detcov_spec as AD
import _assoc_spec as A
import _detect_noise_spec as DN
import _evidence_spec as E
import _fov_spec as V
import _merge_spec as M
import _refine_spec as R
import _sight_spec as S

F = np.float32


class NotReady(Exception):
    """The frame the session refuses with SLAM_ERR_NOT_READY before its first launch."""


def _at(v, f):
    return v(f) if callable(v) else v


def _is_meas_var(cov, meas_var):
    return F(cov[0]) == F(meas_var) and F(cov[1]) == F(0.0) and F(cov[2]) == F(meas_var)


def detect(bx, by, detector):
    """The session's detector on one scan -> (zx [k], zy [k], (qxx, qxy, qyy) [k] or None)."""
    fit, noise = detector.get("fit"), detector.get("noise")
    r = DN.detect_noise(bx, by, fit, noise, **(detector.get("params") or {}))
    if noise is None:
        zx, zy, k, _ = r
        return zx[:k].copy(), zy[:k].copy(), None
    zx, zy, q, k, _ = r
    return zx[:k].copy(), zy[:k].copy(), tuple(v[:k].copy() for v in q)


def frame_loop(world, scans, n, frames, *, seed, sigma, meas_var, score_gain, dp, gate, new_gate, create, noise=("iso",), detector=None,
               detections=None, prune=None, sight=None, fov=None, merge_gate=0.0, refine=None, ess=0.0, score=True, restart=()):
    """world: dict(meta, edt, x, y, th, mp[, bx, by]) (the first n particles are used).  scans: one (bx, by) per frame, or None:
    world's bx, by in every frame.  noise: ("iso",), ("cov", (qxx, qxy, qyy)) or ("detcov",).  detector: None or dict(params=dict
    of slam_detect_params fields, fit=None | (radius, spread_tol), noise=None | (range_var, bearing_var, lateral_var)).
    detections(f) (detector None) -> (zx, zy), (zx, zy, (qxx, qxy, qyy)) or None.  prune: (hit, miss, cmax, view_range); sight:
    (bins, margin); fov: (lo, hi) diamond-angle bounds; merge_gate: 0 = off; refine: (step_xy, step_theta, sweeps); ess: the
    resample gate.  noise, prune, sight, fov, merge_gate, gate and new_gate may each be a function of the frame number.  restart:
    the frames in front of which slam_pf_assoc_set(0, ..) was called and everything was switched on again.
    -> one dict per frame: pose [3][n], map [n][5][L] and ev [n][L] with the frame's resample applied; logw, anc, resampled; and,
    indexed like logw (None on a frame without the stage): assoc, stats, ev_stage (the evidence between its stage and the merge), ev_raw, ev_stats, spared, outside, merge_stats; det =
    (zx, zy, covs or None) and table (the sight table)."""
    import oracle

    x, y, th, mp = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th", "mp"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled, out = None, None, True, []
    ev, was_on = None, False
    for f in range(frames):
        nz, pr, sg, fv, mg = (_at(v, f) for v in (noise, prune, sight, fov, merge_gate))
        g, ng = _at(gate, f), _at(new_gate, f)
        if nz[0] == "cov" and _is_meas_var(nz[1], meas_var):
            nz = ("iso",)
        if pr and (not was_on or f in restart):
            ev = E.evidence_init(mp, pr[2])   # slam_pf_prune_set: the maps that are there are trusted (indexed like mp: before the pending gather)
        was_on = bool(pr)
        bx, by = scans[f] if scans is not None else (world["bx"], world["by"])
        # the detections: refused before anything of the frame runs
        if detector is not None:
            det = detect(bx, by, detector)
        else:
            det = detections(f)
            if det is not None and len(det) == 2:
                det = (det[0], det[1], None)
        if det is not None and nz[0] == "detcov" and det[2] is None:
            raise NotReady(f"frame {f}: per-detection covariances are in force and the detections carry none")
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, _at(dp, f), sigma, seed, f)
        if not score:
            sc = np.zeros(n, np.float32)
        elif refine:
            x, y, th, sc, _ = R.refine(oracle, world["meta"], world["edt"], bx, by, x, y, th, *refine)
        else:
            sc, _ = oracle.score_poses_det(world["meta"], world["edt"], bx, by, x, y, th)
        assoc = stats = ev_stats = ev_stage = spared = outside = merge_stats = T = None
        if det is None:   # no hand-over: maps and evidence follow their particles, the weights are the score's
            if anc is not None:
                mp = mp[anc]
                ev = ev[anc] if pr else ev
            ll = None
        else:
            zx, zy, covs = det
            K = len(zx)
            if nz[0] == "iso":
                assoc, stats = A.associate(mp, x, y, th, anc, zx, zy, meas_var, g, ng, create)
                mp, ll = A.update(mp, x, y, th, anc, assoc, zx, zy, meas_var)
            elif nz[0] == "cov":
                assoc, stats = AA.associate(mp, x, y, th, anc, zx, zy, nz[1], g, ng, create)
                mp, ll = AA.update(mp, x, y, th, anc, assoc, zx, zy, nz[1])
            else:
                assoc, stats = AD.associate(mp, x, y, th, anc, zx, zy, covs, g, ng, create)
                mp, ll = AD.update(mp, x, y, th, anc, assoc, zx, zy, covs)
            if pr and sg:
                T = S.table(bx, by, sg[0])   # of THIS frame's scan, in front of the stage that reads it
            if pr and fv:
                mp, ev, ev_stats, spared, outside = V.evidence(mp, x, y, th, anc, assoc, K, ev, *pr, fv[0], fv[1], T, sg[1] if sg else None)
                spared = spared if sg else None
            elif pr and sg:
                mp, ev, ev_stats, spared = S.evidence(mp, x, y, th, anc, assoc, K, ev, *pr, T, sg[1])
            elif pr:
                mp, ev, ev_stats = E.evidence(mp, x, y, anc, assoc, K, ev, *pr)
            ev_stage = ev if pr else None
            if mg:
                mp, mev, merge_stats = M.merge(mp, assoc, K, mg, ev if pr else None, pr[2] if pr else None)
                ev = mev if pr else ev
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled,
                        assoc=assoc, stats=stats, ev=ev[anc] if pr else None, ev_raw=ev if pr else None, ev_stats=ev_stats, ev_stage=ev_stage, det=det,
                        spared=spared, table=T, outside=outside, merge_stats=merge_stats))
    return out
