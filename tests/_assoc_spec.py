"""The specification of data association ("Data association"; include/slam_hip.h: slam_associate_dev,
slam_ekf_update_assoc_dev, slam_pf_assoc_set) in numpy float32, one rounded operation per line.  TEST INFRASTRUCTURE shared by
test_assoc_spec_cpu.py, test_assoc_behaviour_cpu.py and the GPU tests.  It uses the CPU oracle's deterministic sine / cosine,
its landmark update (oracle/slam_oracle_pf.c: orc_ekf_update) and numpy's float32 division, and nothing of the package.

Detections are points (zx_k, zy_k) in the sensor frame WITHOUT identity, k < K <= 64.  Every particle decides for itself which of
its landmarks each detection belongs to (the gated nearest neighbour in the Mahalanobis term of the update's own likelihood, one
detection per landmark and one landmark per detection) and which detections start a new landmark in a slot not seen so far.
"""
import numpy as np

import oracle

F = np.float32
NONE = 255             # SLAM_ASSOC_NONE
MAX_DETECTIONS = 64    # SLAM_MAX_DETECTIONS


def observed_point(zx, zy, s, c, px, py):
    """w = t + H^T z, exactly as ekf_particle / ekf_first_sighting."""
    t = c * zx
    u = s * zy
    t = t + u
    wx = px + t
    t = c * zy
    u = s * zx
    t = t - u
    wy = py + t
    return wx, wy


def shared(p, meas_var):
    """p [n][5][L] priors -> (seen, mx, my, i00, i01, i11), [n][L] each: which landmarks take part (not P_xx < 0) and
    (P + q I)^-1, the operations of ekf_det_terms and ekf_shared_from."""
    q = F(meas_var)
    mx, my, pxx, pxy, pyy = (p[:, j] for j in range(5))
    seen = ~(pxx < 0)
    a = pxx + q
    cc = pyy + q
    t = a * cc
    u = pxy * pxy
    det = t - u
    idet = F(1.0) / det
    i00 = cc * idet
    i01 = (-pxy) * idet
    i11 = a * idet
    return seen, mx, my, i00, i01, i11


def cost(sh, wx, wy):
    """m(l, k) of one detection k for every landmark: sh from shared(), wx / wy [n][1] -> [n][L]: the Mahalanobis term of the
    likelihood, the operations of ekf_particle."""
    _, mx, my, i00, i01, i11 = sh
    dx = wx - mx
    dy = wy - my
    t = i00 * dx
    u = i01 * dy
    t0 = t + u
    t = i01 * dx
    u = i11 * dy
    t1 = t + u
    t = dx * t0
    u = dy * t1
    return t + u


def associate(map_in, x, y, th, anc, zx, zy, meas_var, gate, new_gate, create, L=None, assoc_stride=None):
    """map_in: float32 [rows][5][plane_stride >= L]; particle i reads row anc[i] (anc None: i).  zx, zy: the K detections.
    -> (assoc uint8 [n][assoc_stride]: entry l = the detection landmark l of particle i takes, 255 = none; stats int32 [n][3] =
    matched, created, dropped)."""
    map_in = np.ascontiguousarray(map_in, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, np.float32), np.ascontiguousarray(zy, np.float32)
    n, K = len(x), len(zx)
    L = map_in.shape[2] if L is None else L
    stride = L if assoc_stride is None else assoc_stride
    gate, new_gate = F(gate), F(new_gate)
    assert K <= MAX_DETECTIONS and stride >= L and np.isfinite(gate) and gate > 0 and new_gate >= gate and meas_var > 0
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    assoc = np.full((n, stride), NONE, np.uint8)
    stats = np.zeros((n, 3), np.int32)
    if K == 0:
        return assoc, stats
    s, c = oracle.det_sincos(th)
    col = lambda a: a[:, None]
    # a. world-frame points, once per (particle, detection)
    wx, wy = observed_point(zx[None, :], zy[None, :], col(s), col(c), col(x), col(y))
    # b. what the seen landmarks share over the detections, then the cost of every (landmark, detection) pair, k by k
    # c. the landmark chooses: its cheapest detection, the lowest k on ties (a strict "<" walking k upwards from +inf: NaN never wins)
    best = np.full((n, L), np.inf, np.float32)
    bk = np.zeros((n, L), np.int64)
    near = np.zeros((n, K), bool)   # (for e: some seen landmark lies within new_gate of detection k)
    with np.errstate(all="ignore"):
        sh = shared(map_in[src][:, :, :L], meas_var)
        seen = sh[0]
        for k in range(K):
            m = cost(sh, wx[:, k:k + 1], wy[:, k:k + 1])
            take = m < best
            best = np.where(take, m, best)
            bk = np.where(take, k, bk)
            near[:, k] = (seen & (m <= new_gate)).any(axis=1)
    cand = seen & (best >= 0) & (best <= gate)
    # d. the detection chooses: among the candidates that chose it the cheapest, the lowest l on ties (argmin: the first minimum)
    matched = np.zeros((n, K), bool)
    rows_i = np.arange(n)
    for k in range(K):
        mine = cand & (bk == k)
        has = mine.any(axis=1)
        if L == 0 or not has.any():
            continue
        l = np.argmin(np.where(mine, best, np.inf), axis=1)
        assoc[rows_i[has], l[has]] = k
        matched[:, k] = has
    stats[:, 0] = matched.sum(axis=1)
    # e. new landmarks: unmatched detections with no seen landmark within new_gate take the unseen slots, both in ascending order
    if create:
        new = ~matched & ~near
        for i in np.flatnonzero(new.any(axis=1)):
            slots = np.flatnonzero(~seen[i])
            ks = np.flatnonzero(new[i])
            cnt = min(len(slots), len(ks))
            assoc[i, slots[:cnt]] = ks[:cnt]
            stats[i, 1] = cnt
    stats[:, 2] = K - stats[:, 0] - stats[:, 1]
    return assoc, stats


def update(map_in, x, y, th, anc, assoc, zx, zy, meas_var, L=None, in_place=False):
    """The landmark update under a per-particle table: particle i gets orc_ekf_update with its own observation list
    {(l, z[assoc[i][l]]) : assoc[i][l] != 255}.  Out of place row i starts as a copy of row anc[i] (anc None: i); in place (anc must
    be None) the same on row i.  -> (map_out [n][5][plane_stride], loglik [n])."""
    assert not (in_place and anc is not None)
    map_in = np.ascontiguousarray(map_in, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, np.float32), np.ascontiguousarray(zy, np.float32)
    n = len(x)
    L = map_in.shape[2] if L is None else L
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    out = np.empty((n,) + map_in.shape[1:], np.float32)
    ll = np.empty(n, np.float32)
    for i in range(n):
        ids = np.flatnonzero(assoc[i, :L] != NONE).astype(np.int32)
        k = assoc[i, ids].astype(np.int64)
        r, l1 = oracle.ekf_update(map_in[src[i]:src[i] + 1], x[i:i + 1], y[i:i + 1], th[i:i + 1], None, ids, zx[k], zy[k], meas_var)
        out[i], ll[i] = r[0], l1[0]
    return out, ll


def frame_loop(world, n, frames, *, seed, sigma, meas_var, score_gain, dp, detections, gate, new_gate, create, ess=0.0, refine=None,
               score=True):
    """The session's frame loop restated from the oracle's stage functions: motion, then score or refine, then associate, then
    update, then weights, then gate, then resample — the executable statement of what a rows session does once slam_pf_assoc_set
    was called.  world: dict(meta, edt, bx, by, x, y, th, mp) (the first n particles are used); detections(f) -> (zx, zy);
    ess: the resample gate (0: every frame resamples); refine: (step_xy, step_theta, sweeps) or None; score = False: a zero
    scan-match score (a drive without a grid; the CPU behaviour test).
    -> one dict per frame: pose [3][n] and map [n][5][L] with the frame's resample applied (what slam_pf_get_poses_host /
    slam_pf_get_map_host return), logw, anc, resampled, and assoc / stats indexed like logw (before the gather)."""
    import _refine_spec as R

    x, y, th, mp = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th", "mp"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled, out = None, None, True, []
    for f in range(frames):
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, dp(f) if callable(dp) else dp, sigma, seed, f)
        if not score:
            sc = np.zeros(n, np.float32)
        elif refine:
            x, y, th, sc, _ = R.refine(oracle, world["meta"], world["edt"], world["bx"], world["by"], x, y, th, *refine)
        else:
            sc, _ = oracle.score_poses_det(world["meta"], world["edt"], world["bx"], world["by"], x, y, th)
        zx, zy = detections(f)
        assoc, stats = associate(mp, x, y, th, anc, zx, zy, meas_var, gate, new_gate, create)
        mp, ll = update(mp, x, y, th, anc, assoc, zx, zy, meas_var)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled,
                        assoc=assoc, stats=stats))
    return out
