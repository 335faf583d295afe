"""tests/_assoc_weight_spec.py on the CPU.  (1) With the constants at 0 its frame loop — a copy of _pipeline_spec.frame_loop with
one step added — returns, bit for bit and key by key, what that loop returns on the pipeline test's eight combinations.  (2) The
miss count it reads off the evidence stage's inputs and outputs is the stage's own predicate: miss_now of _evidence_spec summed
per particle, minus what line of sight spared and the arc left outside; and the scenes hold every kind of count.  (3) The
arithmetic's corners.  (4) What the spec refuses."""
import types

import numpy as np
import pytest

import _assoc_weight_scenes as WS
import _assoc_weight_spec as W
import _pipeline_scenes as SC
from test_pipeline_spec_cpu import same

F = np.float32


@pytest.fixture(scope="module")
def world(orc):
    return SC.make_world()


# ------------------------------------------------------------------ 1. zero constants: the copy is the loop it copies
@pytest.mark.parametrize("name", list(SC.COMBOS))
def test_zero_constants_are_the_pipeline_loop(world, name):
    want = SC.reference(world, name)
    got = WS.run(world, dict(SC.COMBOS[name], assoc_weight=(0.0, 0.0, 0.0)))
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) | {"missed", "terms"}
        for k, v in w.items():
            assert same(g[k], v), f"{name}: frame {f}: {k}"
        assert g["terms"] is not None and not g["terms"].any() and not np.signbit(g["terms"]).any()
    off = WS.run(world, SC.COMBOS[name], frames=3)   # ... and with the switch off
    assert all(same(g["logw"], w["logw"]) and g["terms"] is None for g, w in zip(off, want))


# ------------------------------------------------------------------ 2. the miss count against the predicate
def plain_miss_now(map_rows, x, y, assoc, K, view_range):
    """_evidence_spec.evidence's own lines up to miss_now, summed per particle."""
    n, L = len(x), map_rows.shape[2]
    with np.errstate(all="ignore"):
        range2 = F(view_range) * F(view_range)
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
    return miss_now.sum(axis=1)


def recorded(monkeypatch):
    """The evidence stages of the loop under test, recording per call (form, plain miss_now per particle, spared, outside)."""
    calls = []

    def plain(mp, x, y, anc, assoc, K, ev, hit, miss, cmax, view_range):
        r = W.P.E.evidence(mp, x, y, anc, assoc, K, ev, hit, miss, cmax, view_range)
        calls.append(("plain", plain_miss_now(mp, x, y, assoc, K, view_range), 0, 0))
        return r

    def sight(mp, x, y, th, anc, assoc, K, ev, hit, miss, cmax, view_range, T, margin):
        r = W.P.S.evidence(mp, x, y, th, anc, assoc, K, ev, hit, miss, cmax, view_range, T, margin)
        calls.append(("sight", plain_miss_now(mp, x, y, assoc, K, view_range), r[3], 0))
        return r

    def fov(mp, x, y, th, anc, assoc, K, ev, hit, miss, cmax, view_range, lo, hi, T, margin):
        r = W.P.V.evidence(mp, x, y, th, anc, assoc, K, ev, hit, miss, cmax, view_range, lo, hi, T, margin)
        calls.append(("fov+sight" if T is not None else "fov", plain_miss_now(mp, x, y, assoc, K, view_range), r[3], r[4]))
        return r

    monkeypatch.setattr(W, "E", types.SimpleNamespace(evidence=plain, evidence_init=W.P.E.evidence_init))
    monkeypatch.setattr(W, "S", types.SimpleNamespace(evidence=sight, table=W.P.S.table))
    monkeypatch.setattr(W, "V", types.SimpleNamespace(evidence=fov))
    return calls


FORMS = {"plain": dict(), "sight": dict(sight=SC.SIGHT), "fov": dict(fov=True), "fov+sight": dict(sight=SC.SIGHT, fov=True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_missed_is_the_stages_own_predicate(world, monkeypatch, form):
    calls = recorded(monkeypatch)
    got = WS.run(world, dict(detections=SC.without_cov, prune=SC.PRUNE, merge_gate=SC.MERGE_GATE, assoc_weight=WS.CONSTS, **FORMS[form]))
    assert len(calls) == SC.FRAMES and all(c[0] == form for c in calls)
    spared = outside = 0
    for f, (g, (_, plain, sp, out)) in enumerate(zip(got, calls)):
        assert g["missed"].dtype == np.int32 and np.array_equal(g["missed"], plain - sp - out), f"{form}: frame {f}"
        assert np.all(g["missed"] <= plain)
        assert np.array_equal(g["missed"] >= g["ev_stats"][:, 0], np.ones(SC.N, bool))   # every pruned landmark was a miss
        spared, outside = spared + int(np.sum(sp)), outside + int(np.sum(out))
    assert any(g["missed"].any() for g in got) and any(g["stats"][:, 1].any() for g in got)
    assert ("sight" not in form or spared > 0) and ("fov" not in form or outside > 0)


def test_without_pruning_nothing_is_missed(world):
    got = WS.run(world, dict(detections=SC.without_cov, merge_gate=SC.MERGE_GATE, assoc_weight=WS.CONSTS), frames=4)
    inert = WS.run(world, dict(detections=SC.without_cov, merge_gate=SC.MERGE_GATE, assoc_weight=(WS.CONSTS[0], WS.CONSTS[1], 0.0)), frames=4)
    for g, w in zip(got, inert):
        assert g["missed"] is None and same(g["logw"], w["logw"]) and same(g["terms"], w["terms"])   # log_miss is inert


def test_the_scenes_hold_every_count(world):
    """Conditions on the inputs: a miss, a creation, a drop from the band between the gates, a drop because no slot is left."""
    band = WS.reference(world, "band between the gates")
    assert any(g["missed"].any() for g in band) and any(g["stats"][:, 1].any() for g in band)
    # dropped in a particle that has free slots behind the frame: only the band can have dropped it
    assert any(np.any((g["stats"][:, 2] > 0) & (g["ev_stats"][:, 1] + g["ev_stats"][:, 0] < SC.L)) for g in band)
    small = WS.small_world(world)
    slots = WS.run(small, dict(detections=SC.without_cov, prune=SC.PRUNE, assoc_weight=WS.CONSTS), frames=4)   # gate == new_gate: no band
    full = [g for g in slots if np.any(g["stats"][:, 2] > 0)]
    # ... in particles whose every slot was seen behind the update (pruned + seen after pruning): no slot was left
    assert full and all(np.all((g["ev_stats"][:, 0] + g["ev_stats"][:, 1])[g["stats"][:, 2] > 0] == WS.SLOTS_L) for g in full)
    off = WS.run(small, dict(detections=SC.without_cov, prune=SC.PRUNE), frames=4)
    assert any(not same(g["logw"], w["logw"]) for g, w in zip(slots, off))           # and the drops weigh
    for g in band + slots:                                                            # the terms are the six operations
        if g["terms"] is not None:
            ll, t = W.add(np.zeros(SC.N, F), g["stats"], g["missed"], *WS.CONSTS)
            assert same(t, g["terms"]) and same(ll, t + F(0))


# ------------------------------------------------------------------ 3. the arithmetic's corners
def test_order_and_corners():
    stats = np.array([[0, 3, 5], [0, 64, 64], [0, 0, 0], [0, 1, 0]], np.int32)
    missed = np.array([7, 40, 0, 0], np.int32)
    ll = np.array([-1.25, 0.5, -3.0, 2.0], F)
    c = (F(-0.1), F(-0.7), F(-1.3))
    out, t = W.add(ll, stats, missed, *c)
    for i in range(4):
        a = F(stats[i, 1]) * c[0]
        b = F(stats[i, 2]) * c[1]
        a = F(a + b)
        b = F(missed[i]) * c[2]
        a = F(a + b)
        assert t[i] == a and out[i] == F(ll[i] + a)
    out, t = W.add(ll, stats, missed, -3.0e38, 0.0, -0.0)     # overflow: -inf, never NaN
    assert t[1] == -np.inf and out[1] == -np.inf and t[0] == -np.inf and t[2] == 0 and np.isfinite(t[3]) and not np.isnan(out).any()
    out, t = W.add(ll, stats, None, -0.0, -0.0, -0.0)         # -0 constants: t = -0, ll' = ll
    assert np.signbit(t).all() and same(out, ll)
    out, t = W.add(ll, stats, missed, -1e-45, 0.0, 0.0)       # a denormal stays one
    assert t[0] == F(3) * F(-1e-45) and t[0] != 0 and same(out, ll)
    assert same(W.missed_of(np.array([[3, 2, 0]], np.uint8), None, np.array([[2, 0, 0]], np.uint8),
                            np.array([[[0] * 3, [0] * 3, [1, 1, -1], [0] * 3, [0] * 3]], F),
                            np.array([[[0] * 3, [0] * 3, [1, 1, -1], [0] * 3, [0] * 3]], F)), np.array([2], np.int32))
    # a landmark pruned at evidence 0 (miss > c = 0): the byte does not move, the slot does
    assert same(W.missed_of(np.array([[0]], np.uint8), None, np.array([[0]], np.uint8), np.array([[[0], [0], [1], [0], [0]]], F),
                            np.array([[[0], [0], [-1], [0], [0]]], F)), np.array([1], np.int32))


# ------------------------------------------------------------------ 4. what the spec refuses
@pytest.mark.parametrize("bad", [1e-30, 1.0, float("nan"), float("inf"), float("-inf"), -1e39])
@pytest.mark.parametrize("slot", [0, 1, 2])
def test_constants_are_checked(bad, slot):
    c = [-1.0, -1.0, -1.0]
    c[slot] = bad
    with pytest.raises(ValueError):
        W.check_constants(*c)
    with pytest.raises(ValueError):
        W.add(np.zeros(1, F), np.zeros((1, 3), np.int32), None, *c)


def test_the_loop_checks_them_too(world):
    with pytest.raises(ValueError):
        WS.run(world, dict(detections=SC.without_cov, assoc_weight=(0.5, 0.0, 0.0)), frames=1)
    assert W.check_constants(0, -0.0, -3.0e38) == (F(0), F(-0.0), F(-3.0e38))
