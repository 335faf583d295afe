"""The flaw the switch removes, and its remedy, derived rather than tuned ("The unexplained").

Eight landmarks, each seen once: P = q I with q = meas_var = 0.09 (a 0.3 m detector).  Eight detections lie exactly on them for
the first half of 64 particles; the second half stands 5 m away, so every detection lies beyond new_gate of every landmark
(25 / 0.18 = 139 against 9.21) and starts a landmark in one of eight free slots.  The score is off: the weights are the landmark
likelihood alone.

A match contributes -m/2 - log(2 pi (p + q)) = -log(2 pi 0.18) = -0.123 at m = 0: negative, because p + q = 0.18 > 1 / (2 pi).
Eight of them: -0.98.  A particle that matches nothing scores 0 and WINS.  With log_new = -4 it pays -32 and loses.  With pruning,
log_new = 0 and log_miss = -2 it pays for eight landmarks in view that took no detection: -16."""
import numpy as np
import pytest

import _assoc_weight_spec as W

F = np.float32
N, L, Q = 64, 16, 0.09
GATE = NEW_GATE = 9.21
KW = dict(seed=3, sigma=(0.0, 0.0, 0.0), meas_var=Q, score_gain=0.0, dp=[0.0, 0.0, 0.0], gate=GATE, new_gate=NEW_GATE, create=1, score=False)
LM = np.stack([np.zeros(8), 2.0 * np.arange(8) - 7.0], 1).astype(F)     # on a line, 2 m apart


def world():
    mp = np.zeros((N, 5, L), F)
    mp[:, 2] = -1.0
    mp[:, 0, :8], mp[:, 1, :8] = LM[:, 0], LM[:, 1]
    mp[:, 2, :8], mp[:, 3, :8], mp[:, 4, :8] = Q, 0.0, Q                # seen once: P = q I
    x = np.zeros(N, F)
    x[N // 2:] = 5.0                                                     # the displaced half
    return dict(x=x, y=np.zeros(N, F), th=np.zeros(N, F), mp=mp)


def frame(**kw):
    """One frame; the detections are the landmarks as the TRUE half sees them (pose 0: sensor frame = world frame)."""
    return W.frame_loop(world(), [(None, None)], N, 1, detections=lambda f: (LM[:, 0].copy(), LM[:, 1].copy()), **kw, **KW)[0]


@pytest.fixture(scope="module")
def off(orc):
    return frame()


def test_the_setup_is_the_one_described(off):
    true, far = slice(0, N // 2), slice(N // 2, N)
    assert np.all(off["stats"][true] == (8, 0, 0)) and np.all(off["stats"][far] == (0, 8, 0))
    assert 0.09 + 0.09 > 1 / (2 * np.pi)


def test_switch_off_the_wrong_particles_win(off):
    """(passes without the feature: this is the flaw)"""
    lw = off["logw"]
    assert lw[N // 2:].min() > lw[:N // 2].max()
    assert abs(float(lw[0]) - 8 * -np.log(2 * np.pi * 0.18)) < 1e-3 and np.all(lw[N // 2:] == 0)


def test_switch_on_the_true_particles_win(orc):
    on = frame(assoc_weight=(-4.0, 0.0, 0.0))
    lw = on["logw"]
    assert lw[:N // 2].min() > lw[N // 2:].max()
    assert np.all(on["terms"][N // 2:] == -32) and np.all(on["terms"][:N // 2] == 0) and on["missed"] is None


def test_misses_weigh_with_pruning(orc):
    prune = (1, 1, 4, 20.0)                      # every old landmark lies within view_range of the displaced half too
    off = frame(prune=prune)
    on = frame(prune=prune, assoc_weight=(0.0, 0.0, -2.0))
    assert np.all(on["missed"][N // 2:] == 8) and np.all(on["missed"][:N // 2] == 0)
    assert off["logw"][N // 2:].min() > off["logw"][:N // 2].max()     # off: the flaw, with pruning as without
    assert on["logw"][:N // 2].min() > on["logw"][N // 2:].max()       # on: eight misses at -2 against eight matches at -0.123
