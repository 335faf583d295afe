"""The frame of a session that localises in a known map with EVERY switch, composed from the stage specifications (DESIGN.md section
7, "The whole known-map frame"; csrc/pf_session_frame.hip: pf_step_impl, update_rows; csrc/pf_session.hip: known_map_set,
known_map_reseed, slam_pf_known_map_miss_set, slam_pf_detect_noise_set; csrc/pf_session_read.hip).  TEST INFRASTRUCTURE shared by
test_known_pipeline_spec_cpu.py and test_gpu_known_pipeline_session.py.  It adds NO arithmetic: every stage is a function of
tests/_detect_noise_spec.py (through _pipeline_spec.detect), _refine_spec.py, _localise_miss_spec.py (which is _localise_spec.py /
_localise_detcov_spec.py with the misses off), _sight_spec.py, _reseed_spec.py, _reseed_pair_spec.py, _estimate_spec.py,
_spread_spec.py or of the oracle, and what is stated here is only the plumbing between them — which stage runs, in which order,
on which poses, detections, map and scan.

A frame (Session.step), in the order pf_step_impl runs it:

  refusal     under the per-detection form an observing frame whose detections will carry no covariance — the detector is on
              without a noise model, or it is off and the detections the engine holds were uploaded without — raises NotReady
              BEFORE anything runs: the session is as it was (the frame number too)
  detections  the detector on the frame's scan when it is on (what was uploaded is then overwritten), else what the engine holds:
              the last upload, or what the last detector launch left.  A frame with use_observations == 0, and every frame while
              the mode is off, runs neither: the engine keeps the detections it has
  motion      from the pending ancestors — behind a reseed there are none (identity) — under the session's frame number
  score       the scan-match score, or the refinement: every later stage reads the REFINED poses
  localise    in the noise form in force, with or without the misses; the sight table is made from THIS frame's scan, in front of
              the stage that reads it; the clutter and miss terms on the stage's stats and counts
  weights     with the carry of a frame the gate kept — none behind a reseed —, the gate's verdict, the resample

Between frames (Session.reseed) slam_pf_known_map_reseed / _reseed_pairs read the frame's poses through the pending ancestors, the
detections the engine holds NOW and the map as it was given, under the frame number of the NEXT frame (the session's counter
behind the step).  A call with fewer detections than it needs (1; pairs: 2) returns zero counts and changes nothing: the gather
stays pending, `best` still answers.

The switch rules, as the code has them:

  * Replacing the map (either set call, either noise form, any landmark count — also one that needs a larger allocation) keeps
    the misses and the detector, the poses, the pending gather and the weight carry.
  * Switching the map off (rows == NULL) takes the detector and the misses with it; a map set behind it brings neither back.
  * slam_pf_known_map_set (isotropic) drops the detector's noise model; the detector stays on without it.  A later
    slam_pf_known_map_detcov_set does not bring the model back: its first observing frame is refused (NotReady) until
    slam_pf_detect_noise_set gives the model again.
  * A frame refused with NotReady leaves the session as it was: the same step accepted later is the step of a session that
    was never refused.
  * slam_pf_detect_noise_set with a model is refused (InvalidArg) under the isotropic form, the detector without a map;
    slam_pf_known_map_miss_set without a map likewise.  The session is as it was.
  * A reseed while the mode is off is refused (NotReady); nothing moves.
  * A successful reseed clears the pending gather and, under the gate, the weight carry (the next frame weighs as behind a
    resample); the verdict of the frame in front of it is counted into frames_resampled by the call.
  * `best` is refused from a successful reseed until the next step; `mean` and `spread` see equal weights behind a reseed (the
    plain form), the weighted form behind a frame the gate kept, the plain form behind a frame that resampled.
"""
import numpy as np

import _estimate_spec as E
import _localise_miss_spec as MS
import _pipeline_spec as P
import _refine_spec as RF
import _reseed_pair_spec as RP
import _reseed_spec as R
import _sight_spec as S
import _spread_spec as SP

F = np.float32
NotReady = P.NotReady


class InvalidArg(Exception):
    """The call the session refuses with SLAM_ERR_INVALID_ARG; the session is as it was."""


def _at(v, f):
    return v(f) if callable(v) else v


class Session:
    """What a session with n_landmarks == 0 on one GPU holds between its calls, and the calls.  arc: the diamond-angle bounds
    (lo, hi) the misses' field of view comes down to (the library's own, or _fov_spec.bound's)."""

    def __init__(self, world, n, *, seed, sigma, meas_var, score_gain, ess=0.0, refine=None, score=True, arc=None):
        import oracle

        self.o, self.world, self.n = oracle, world, n
        self.seed, self.sigma, self.meas_var, self.score_gain, self.refine, self.score, self.arc = seed, sigma, meas_var, score_gain, refine, score, arc
        self.fq = oracle.ess_frac_q16(ess)
        self.x, self.y, self.th = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th"))
        self.anc, self.carry, self.prev_resampled, self.frame, self.frames_resampled = None, None, True, 0, 0
        self.M = self.form = self.gate = self.log_clutter = self.miss = self.detector = self.held = self.scan = self.logw = None
        self.reseeded, self.prepares = False, 0

    # ---- the switches
    def known_map_set(self, M, form=None, gate=None, log_clutter=None):
        if M is None:
            if self.M is not None:
                self.detector = None
            self.M = self.form = self.miss = None
            return
        self.M, self.form, self.gate, self.log_clutter = np.ascontiguousarray(M, F), form, gate, log_clutter
        self.prepares += int(form == "iso")   # (the prepared map: made at the switch, never inside a frame)
        if form == "iso" and self.detector and self.detector.get("noise") is not None:
            self.detector = dict(self.detector, noise=None)

    def miss_set(self, miss):
        """miss: None (off) or (log_miss, view_range, fov: bool, sight: None or (bins, margin))"""
        if miss is not None and self.M is None:
            raise InvalidArg("the misses need a known map")
        self.miss = miss

    def detect_set(self, detector):
        """detector: None (off) or dict(params, fit=None | (radius, spread_tol), noise=None | (range_var, bearing_var, lateral_var))"""
        if detector is None:
            self.detector = None
            return
        if self.M is None:
            raise InvalidArg("the detector needs a known map")
        if self.form == "iso" and detector.get("noise") is not None:
            raise InvalidArg("the isotropic form takes no noise model")
        self.detector = dict(detector)

    def upload(self, det):
        self.held = (det[0], det[1], det[2] if len(det) == 3 else None)

    def scan_set(self, bx, by):
        self.scan = (bx, by)

    # ---- the frame
    def step(self, dp, observing):
        o, n = self.o, self.n
        localise = self.M is not None and bool(observing)
        if localise and self.form == "detcov":
            if (self.detector.get("noise") is None) if self.detector else (self.held is None or self.held[2] is None):
                raise NotReady(f"frame {self.frame}: per-detection covariances are in force and the detections carry none")
        bx, by = self.scan
        if self.detector and localise:
            self.held = P.detect(bx, by, self.detector)
        if self.fq and self.anc is not None:
            self.frames_resampled += int(self.prev_resampled)   # the host looks at the last frame's verdict now
        x, y, th = o.motion_sample(self.x, self.y, self.th, self.anc, n, 0, dp, self.sigma, self.seed, self.frame)
        if not self.score:
            sc = np.zeros(n, np.float32)
        elif self.refine:
            x, y, th, sc, _ = RF.refine(o, self.world["meta"], self.world["edt"], bx, by, x, y, th, *self.refine)
        else:
            sc, _ = o.score_poses_det(self.world["meta"], self.world["edt"], bx, by, x, y, th)
        assoc = stats = ll = missed = spared = outside = T = None
        if localise:
            zx, zy, covs = self.held
            view = None
            if self.miss is not None:
                log_miss, view_range, fov, sight = self.miss
                T = S.table(bx, by, sight[0]) if sight else None   # of THIS frame's scan
                view = (view_range, tuple(self.arc) if fov else None, sight[1] if sight else None)
            assoc, stats, ll, missed, spared, outside = MS.localise(self.M, x, y, th, zx, zy, covs if self.form == "detcov" else self.meas_var,
                                                                    self.gate, self.log_clutter, self.miss[0] if self.miss is not None else 0.0, view, T)
        logw, m = o.logweight_carry(sc, ll, self.score_gain, None if self.prev_resampled else self.carry)
        wq, _ = o.quantise_weights(logw, m)
        s16, q16 = o.ess_terms(wq)
        self.prev_resampled = o.ess_resample(s16, q16, n, self.fq) if self.fq else True
        self.carry = o.weight_carry(logw, m)
        self.anc = o.resample(wq, self.seed, self.frame) if self.prev_resampled else np.arange(n, dtype=np.int32)
        self.x, self.y, self.th, self.logw = x, y, th, logw
        self.frame += 1
        self.reseeded = False
        return dict(pose=self.population(), logw=logw, anc=self.anc, resampled=self.prev_resampled, assoc=assoc, stats=stats, ll=ll,
                    missed=missed, spared=spared, outside=outside, table=T, det=self.held,
                    launched=self.launched(localise, ran=self.detector if localise else None, table=T is not None))

    def moved(self):
        """The launches of the last step or reseed call (`launched`)."""
        return self._moved

    def launched(self, localise=False, ran=None, table=False, reseed=None):
        """The launches since the last record, by the engine's counters: the map prepared (every isotropic set), the stage in its
        form (iso, detcov or — either noise form — miss), the weight terms, the sight table, the detector (and its fit and its
        model), the two reseeds.  Everything else: none."""
        miss = localise and self.miss is not None
        out = dict(prepare=self.prepares, iso=int(localise and not miss and self.form == "iso"), detcov=int(localise and not miss and self.form == "detcov"),
                   miss=int(miss), weight=int(localise and (self.log_clutter != 0 or (miss and self.miss[0] != 0))), sight=int(table),
                   detect=int(ran is not None), fit=int(bool(ran and ran.get("fit"))), model=int(bool(ran and ran.get("noise"))),
                   single=int(reseed == "single"), pairs=int(reseed == "pairs"))
        self.prepares = 0
        self._moved = out
        return out

    # ---- between frames
    def reseed(self, call):
        """call: ("single", fraction) or ("pairs", fraction, tol, min_sep) -> the counts (a tuple of 2 or 4)."""
        if self.M is None:
            raise NotReady("reseed: the mode is off")
        if self.held is None:
            raise NotReady("reseed: no detections were handed over")
        pairs = call[0] == "pairs"
        zx, zy, _ = self.held
        if len(zx) < (2 if pairs else 1):
            self.launched()
            return (0,) * (4 if pairs else 2)
        self.launched(reseed=call[0])
        if pairs:
            x, y, th, _, counts = RP.reseed_pairs(self.M, self.x, self.y, self.th, self.anc, zx, zy, 0, self.seed, self.frame, *call[1:])
        else:
            x, y, th, _, counts = R.reseed(self.M, self.x, self.y, self.th, self.anc, zx, zy, 0, self.seed, self.frame, call[1])
        if self.fq and self.anc is not None:
            self.frames_resampled += int(self.prev_resampled)   # the verdict of the frame in front, before the gate forgets it
        self.x, self.y, self.th = x, y, th
        self.anc, self.prev_resampled, self.reseeded = None, True, True   # nothing is pending, no weight is carried
        return tuple(int(v) for v in counts)

    def pending(self):
        """Is a gather pending (slam_pf_device_view: anc)?"""
        return self.anc is not None

    def population(self):
        """The poses as the host reads them: through the pending gather."""
        a = slice(None) if self.anc is None else self.anc
        return np.stack([self.x[a], self.y[a], self.th[a]])

    def reads(self, ref):
        """-> dict(mean float32 [3], spread (pose, cov [6], heading_r), best (pose, log-weight, index) or None: refused)."""
        px, py, pth = self.population()
        kept = bool(self.fq) and self.anc is not None and not self.prev_resampled
        w16 = E.weights16(self.logw)[0] if kept else None
        sp = SP.spread_spec(px, py, pth, None, ref, self.n, w16)
        if w16 is not None and sum(int(v) for v in w16) <= 0:
            w16 = None
        best = None
        if not self.reseeded and self.logw is not None:
            best = E.best_spec(self.logw, self.x, self.y, self.th)
        verdict = bool(self.prev_resampled) if self.fq and self.anc is not None else None   # (slam_resample_happened_host)
        return dict(mean=E.mean_spec(px, py, pth, None, ref, self.n, w16)[0], spread=sp[:3], best=best, verdict=verdict,
                    frames_resampled=self.frames_resampled)


def drive(ses, scans, frames, *, dp, gate, log_clutter, known_map, noise=("iso",), detector=None, detections=None, miss=None,
          observing=None, reseed_after=None, restart=(), redetect=(), regive=(), tries=None, ref=0.0):
    """The calls a host makes on `ses` — a Session above, or anything with its methods — for a schedule given as functions of the
    frame number, and what it reads behind each.  A switch is given when its value changes (and all of them behind a restart):
      known_map(f) -> M or None (off); noise(f) -> ("iso",) | ("detcov",): either change is ONE set call in the frame's form
      miss(f) -> None | (log_miss, view_range, fov, sight);  detector(f) -> None | dict
      detections(f) -> what is uploaded in front of the frame while the detector is off (None: nothing)
      observing(f) -> use_observations (default: the detector is on, or something was uploaded)
      reseed_after(f) -> None, a call or a list of calls, made behind the frame with no step between them
      restart: frames in front of which the map is switched off and everything given again
      redetect: frames in front of which the detector is given again as it is asked for
      regive: frames whose step is refused (NotReady) — it must be — and asked again after the detector was given again
      tries(f) -> refused calls made in front of the frame: "model" (the detector with a noise model: under the isotropic form),
                  "reseed-off" (a reseed behind the switch-off of a restart), "miss-off" (the misses behind that switch-off)
    -> a list of events: ("refused", f, what), ("frame", f, record, reads, moved), ("reseed", f, call, counts, population, reads,
    pending: a gather is still pending — the call was a no-op, moved); moved: Session.launched."""
    ev, prev = [], dict(M=None, nz=None, ms=None, dt=None)
    for f in range(frames):
        M, nz, ms, dt = _at(known_map, f), _at(noise, f)[0], _at(miss, f), _at(detector, f)
        asked = list(tries(f)) if tries else []
        if f in restart:
            ses.known_map_set(None)
            for what, call in (("reseed-off", lambda: ses.reseed(("single", 0.5))), ("miss-off", lambda: ses.miss_set((-1.0, 1.0, False, None)))):
                if what in asked:
                    try:
                        call()
                    except (NotReady, InvalidArg) as err:
                        ev.append(("refused", f, what, type(err).__name__))
                    else:
                        raise AssertionError(f"frame {f}: {what} was accepted")
            prev = dict(M=None, nz=None, ms=None, dt=None)
        if M is not prev["M"] or (M is not None and nz != prev["nz"]):
            ses.known_map_set(M, nz, gate, log_clutter)
        if M is None:
            ms = dt = None
        if ms != prev["ms"]:
            ses.miss_set(ms)
        if dt != prev["dt"] or (dt is not None and f in redetect):
            ses.detect_set(dt)
        if "model" in asked:
            try:
                ses.detect_set(dict(dt or {"params": {}}, noise=(1e-3, 1e-4, 0.0)))
            except InvalidArg:
                ev.append(("refused", f, "model", "InvalidArg"))
            else:
                raise AssertionError(f"frame {f}: a noise model was accepted")
        prev = dict(M=M, nz=nz, ms=ms, dt=dt)
        ses.scan_set(*scans[f])
        det = detections(f) if detections and dt is None else None
        if det is not None:
            ses.upload(det)
        obs = _at(observing, f) if observing is not None else (dt is not None or det is not None)
        if f in regive:
            try:
                ses.step(_at(dp, f), obs)
            except NotReady:
                ev.append(("refused", f, "frame", "NotReady"))
            else:
                raise AssertionError(f"frame {f}: the frame was accepted")
            ses.detect_set(dt)
        rec = ses.step(_at(dp, f), obs)
        ev.append(("frame", f, rec, ses.reads(ref), ses.moved()))
        calls = reseed_after(f) if reseed_after else None
        if calls is not None:
            for call in (calls if isinstance(calls, list) else [calls]):
                counts = ses.reseed(call)
                ev.append(("reseed", f, call, counts, ses.population(), ses.reads(ref), ses.pending(), ses.moved()))
    return ev


def frame_loop(world, scans, n, frames, *, seed, sigma, meas_var, score_gain, dp, gate, log_clutter, known_map, ess=0.0, refine=None,
               score=True, arc=None, **schedule):
    """`drive` on a Session of this file -> one dict per frame: the record of Session.step (pose [3][n] with the frame's resample
    applied, logw, anc, resampled, assoc, stats, ll, missed, spared, outside, table, det = (zx, zy, covs or None) the engine
    holds), reads (Session.reads behind the step), refused (what was refused in front of it), reseeds (one dict(call, counts,
    reseeded, reads) per call; reseeded None where the call was a no-op), and — the first call's, as _reseed_spec.frame_loop and
    _reseed_pair_spec.frame_loop name them — counts and reseeded.  The Session is returned in the last frame's dict as `session`."""
    ses = Session(world, n, seed=seed, sigma=sigma, meas_var=meas_var, score_gain=score_gain, ess=ess, refine=refine, score=score, arc=arc)
    out, refused = [], []
    for e in drive(ses, scans, frames, dp=dp, gate=gate, log_clutter=log_clutter, known_map=known_map, **schedule):
        if e[0] == "refused":
            refused.append(e[2])
        elif e[0] == "frame":
            out.append(dict(e[2], reads=e[3], refused=refused, reseeds=[], counts=None, reseeded=None))
            refused = []
        else:
            moved = not e[6]
            out[-1]["reseeds"].append(dict(call=e[2], counts=e[3], reseeded=e[4] if moved else None, reads=e[5]))
            if len(out[-1]["reseeds"]) == 1:
                out[-1]["counts"], out[-1]["reseeded"] = np.array(e[3], np.int32), e[4] if moved else None
    out[-1]["session"] = ses
    return out
