"""The specification of the weight of what a frame's association leaves unexplained ("The unexplained";
include/slam_hip.h: slam_assoc_weight_dev, the _missed evidence stages, slam_pf_assoc_weight_set) in numpy float32, one rounded
operation per line.  TEST INFRASTRUCTURE shared by test_assoc_weight_spec_cpu.py, test_assoc_weight_behaviour_cpu.py and the GPU
tests.  It imports the existing specifications and restates nothing of them.

The associating update's log-likelihood sums one term per MATCHED pair.  Here three per-particle counts of the frame enter it too:

  created   stats[i][1] of the frame's association, as it is
  dropped   stats[i][2], as it is: detections between the two gates, and detections no slot was left for
  missed    the slots the frame's evidence stage SCORED AS A MISS in whichever form ran (plain, sight, fov, fov + sight): those
            whose evidence byte it lowered or whose landmark it pruned.  miss >= 1, so every miss does one of the two.  It is
            read off the stage's inputs and outputs (`missed_of`): no second copy of the visibility predicate lives here.  A
            landmark line of sight spared or the arc left outside took no miss and is none.  Pruning off: 0.

With float32 constants log_new, log_clutter, log_miss — each finite and <= 0, else ValueError — `add` is the six operations

  t = F(created) * log_new;  u = F(dropped) * log_clutter;  t = t + u;  u = F(missed) * log_miss;  t = t + u;  ll' = ll + t

and ll' goes to the weights in the place of ll.  The counts are exact in float32 (created, dropped <= 64, missed <= L).  A product
that overflows is -inf and stays -inf (no constant is infinite, so no 0 * inf: never a NaN).  (0, 0, 0) is a valid "on": t = +0
and ll' has the bits of ll.  A non-zero log_miss without pruning is accepted and INERT: nothing scores a miss.  A frame without a
detection hand-over adds nothing; merging, which runs behind the evidence stage, does not change the counts.
"""
import numpy as np

import _pipeline_spec as P

F = np.float32
A, AA, AD, E, M, R, S, V = P.A, P.AA, P.AD, P.E, P.M, P.R, P.S, P.V


def check_constants(log_new, log_clutter, log_miss):
    """-> the three as float32; ValueError for one that is positive, NaN or infinite (after rounding to float32)."""
    with np.errstate(over="ignore"):
        c = tuple(F(v) for v in (log_new, log_clutter, log_miss))
    for name, v in zip(("log_new", "log_clutter", "log_miss"), c):
        if not (np.isfinite(v) and v <= 0):
            raise ValueError(f"{name} = {v}: the log-likelihood of an event must be finite and <= 0")
    return c


def missed_of(ev_in, anc, ev_out, map_in, map_out, L=None):
    """What an evidence stage scored as a miss, from its inputs and outputs: ev_in uint8 [rows][>= L] read behind anc (None: i),
    ev_out uint8 [n][>= L]; map_in / map_out float32 [n][5][>= L] the rows in front of and behind the stage -> int32 [n].
    Only a slot that holds a landmark in map_in can be missed.  (The evidence bytes are a session's: at most cmax — else a hit
    would lower one too.)"""
    map_in, map_out = np.asarray(map_in), np.asarray(map_out)
    n = len(ev_out)
    L = map_in.shape[2] if L is None else L
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    seen_in = ~(map_in[:n, 2, :L] < 0)
    lowered = seen_in & (np.asarray(ev_out)[:, :L] < np.asarray(ev_in)[src][:, :L])
    pruned = seen_in & (map_out[:n, 2, :L] < 0)
    return (lowered | pruned).sum(axis=1).astype(np.int32)


def terms(created, dropped, missed, log_new, log_clutter, log_miss):
    """-> t float32 [n] (missed None: 0)."""
    log_new, log_clutter, log_miss = check_constants(log_new, log_clutter, log_miss)
    created, dropped = np.asarray(created), np.asarray(dropped)
    missed = np.zeros(len(created), np.int32) if missed is None else np.asarray(missed)
    with np.errstate(over="ignore"):
        t = created.astype(F) * log_new
        u = dropped.astype(F) * log_clutter
        t = t + u
        u = missed.astype(F) * log_miss
        t = t + u
    return t


def add(ll, stats, missed, log_new, log_clutter, log_miss):
    """ll float32 [n]; stats int32 [n][3] of the association -> (ll', t)."""
    stats = np.asarray(stats)
    t = terms(stats[:, 1], stats[:, 2], missed, log_new, log_clutter, log_miss)
    with np.errstate(over="ignore"):
        out = np.asarray(ll, F) + t
    return out, t


def frame_loop(world, scans, n, frames, *, seed, sigma, meas_var, score_gain, dp, gate, new_gate, create, noise=("iso",), detector=None,
               detections=None, prune=None, sight=None, fov=None, merge_gate=0.0, refine=None, ess=0.0, score=True, restart=(),
               assoc_weight=None):
    """_pipeline_spec.frame_loop plus exactly one step between the merge and the weights: `add`.  assoc_weight: None (off), or
    (log_new, log_clutter, log_miss), or a function of the frame number that returns either.  Every other argument and every key of
    the result is _pipeline_spec.frame_loop's; the result gains missed int32 [n] (None where no evidence stage ran) and terms
    float32 [n] (None where the step did not run), indexed like logw.

    That loop has no seam between its merge and its weights (the log-likelihood is a local it hands straight to the oracle), so
    the step cannot be injected by wrapping it: its body is COPIED here, every stage still a call into the specification it
    came from.  test_assoc_weight_spec_cpu.py pins the copy to _pipeline_spec.frame_loop with the constants at 0 — bit for bit and
    key by key on the pipeline test's eight combinations."""
    import oracle

    x, y, th, mp = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th", "mp"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled, out = None, None, True, []
    ev, was_on = None, False
    for f in range(frames):
        nz, pr, sg, fv, mg, aw = (P._at(v, f) for v in (noise, prune, sight, fov, merge_gate, assoc_weight))
        g, ng = P._at(gate, f), P._at(new_gate, f)
        if aw is not None:
            aw = check_constants(*aw)
        if nz[0] == "cov" and P._is_meas_var(nz[1], meas_var):
            nz = ("iso",)
        if pr and (not was_on or f in restart):
            ev = E.evidence_init(mp, pr[2])
        was_on = bool(pr)
        bx, by = scans[f] if scans is not None else (world["bx"], world["by"])
        if detector is not None:
            det = P.detect(bx, by, detector)
        else:
            det = detections(f)
            if det is not None and len(det) == 2:
                det = (det[0], det[1], None)
        if det is not None and nz[0] == "detcov" and det[2] is None:
            raise P.NotReady(f"frame {f}: per-detection covariances are in force and the detections carry none")
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, P._at(dp, f), sigma, seed, f)
        if not score:
            sc = np.zeros(n, np.float32)
        elif refine:
            x, y, th, sc, _ = R.refine(oracle, world["meta"], world["edt"], bx, by, x, y, th, *refine)
        else:
            sc, _ = oracle.score_poses_det(world["meta"], world["edt"], bx, by, x, y, th)
        assoc = stats = ev_stats = ev_stage = spared = outside = merge_stats = T = missed = t = None
        if det is None:
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
            mp_in, ev_in = mp, ev   # what the evidence stage reads: the rows the update wrote, last frame's evidence behind anc
            if pr and sg:
                T = S.table(bx, by, sg[0])
            if pr and fv:
                mp, ev, ev_stats, spared, outside = V.evidence(mp, x, y, th, anc, assoc, K, ev, *pr, fv[0], fv[1], T, sg[1] if sg else None)
                spared = spared if sg else None
            elif pr and sg:
                mp, ev, ev_stats, spared = S.evidence(mp, x, y, th, anc, assoc, K, ev, *pr, T, sg[1])
            elif pr:
                mp, ev, ev_stats = E.evidence(mp, x, y, anc, assoc, K, ev, *pr)
            if pr:
                missed = missed_of(ev_in, anc, ev, mp_in, mp)
            ev_stage = ev if pr else None
            if mg:
                mp, mev, merge_stats = M.merge(mp, assoc, K, mg, ev if pr else None, pr[2] if pr else None)
                ev = mev if pr else ev
            if aw is not None:   # THE STEP: between the merge and the weights
                ll, t = add(ll, stats, missed, *aw)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled,
                        assoc=assoc, stats=stats, ev=ev[anc] if pr else None, ev_raw=ev if pr else None, ev_stats=ev_stats, ev_stage=ev_stage, det=det,
                        spared=spared, table=T, outside=outside, merge_stats=merge_stats, missed=missed, terms=t))
    return out
