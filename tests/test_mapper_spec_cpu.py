"""The mapper's frame loop in stage functions (tests/_mapper_spec.py) against the oracle's own loop, and the facts about
the generated cases that tests/test_gpu_mapper.py relies on.  Runs without a GPU.

Every case must exercise what it claims: the conditions below are about the inputs, worked out on the CPU, so a case
cannot silently stop testing its edge.  If one does not hold, the inputs are wrong, not the condition."""
import numpy as np
import pytest

import _mapper_spec as ms
from conftest import bits

_TRACES = {}


def trace(orc, name):
    """Run the spec and orc_slam_* side by side over the case; -> one record per frame (frame 0 = first_frame)."""
    if name in _TRACES:
        return _TRACES[name]
    c = ms.case(orc, name)
    spec = c.spec(orc)
    slam = orc.Slam(c.nbeams, c.angle_min, c.angle_inc, c.orc_params(orc), "window")
    out = []
    for f, r in enumerate(c.frames):
        if f == 0:
            spec.first_frame(r)
            slam.first_frame(r)
        else:
            before = slam.partial_frames()
            pose = spec.next_frame(r)
            assert np.array_equal(bits(pose), bits(slam.next_frame(r))), f"{name}: pose of frame {f}"
            assert spec.partial == (slam.partial_frames() - before == 1), f"{name}: partial flag of frame {f}"
        assert spec.map_n == slam.map_size(), f"{name}: map size after frame {f}"
        assert np.array_equal(bits(spec.map_x), bits(slam.map_x())) and np.array_equal(bits(spec.map_y), bits(slam.map_y()))
        if spec.rebuilt:   # the numpy crop mask is the crop
            assert np.array_equal(bits(spec.map_x[: spec.map_before][spec.crop_keep]), bits(spec.lx))
            assert np.array_equal(bits(spec.map_y[: spec.map_before][spec.crop_keep]), bits(spec.ly))
        out.append(dict(key=spec.key, rebuilt=spec.rebuilt, partial=spec.partial, scan_n=spec.scan_n, map_n=spec.map_n,
                        map_before=spec.map_before, lsize=len(spec.lx), candidates=spec.candidates, appended=spec.appended,
                        hits=spec.hits.copy(), hits_n=spec.hits_n, keep=None if spec.crop_keep is None else spec.crop_keep.copy(),
                        cols=[m.cols for m in spec.meta], rows=[m.rows for m in spec.meta], pose=spec.pose.copy(),
                        map_x=spec.map_x.copy(), map_y=spec.map_y.copy()))
    assert slam.partial_frames() == sum(t["partial"] for t in out)
    slam.close()
    _TRACES[name] = out
    return out


@pytest.mark.parametrize("name", ms.ALL_CASES)
def test_spec_equals_the_oracle_loop(orc, name):
    tr = trace(orc, name)
    assert len(tr) == len(ms.case(orc, name).frames) <= 12
    assert tr[1]["rebuilt"]   # the first frame after first_frame always rebuilds


def test_beam_cases_cover_the_compaction_seams(orc):
    counts = {}
    for name in ms.BEAM_CASES:
        _, n, pat = name.split("-")
        tr = trace(orc, name)
        assert all(t["scan_n"] == tr[0]["scan_n"] > 0 for t in tr)
        assert tr[0]["map_n"] == tr[0]["scan_n"] == int(ms.survivor_patterns(int(n))[pat].sum())
        counts.setdefault(int(n), set()).add(tr[0]["scan_n"])
    assert sorted(counts) == sorted(ms.BEAM_COUNTS)
    every = set().union(*counts.values())
    assert any(c % 64 == 0 for c in every) and any(c % 64 == 1 for c in every)
    assert {1024, 2048, 4096} <= every and {1, 65, 1025, 2049} <= every
    for n, cs in counts.items():
        if n > 1024:
            assert max(cs) > 1024
            assert n - 1024 in cs   # batch 0 empty, batch 1 kept


def test_gate_case_sits_on_the_comparisons(orc):
    c = ms.case(orc, "gate")
    par = c.orc_params(orc)
    ang = c.angles(orc)
    vals = ms.gate_values(par)
    assert vals[0][0] == np.float32(par.range_min) and vals[3][0] == np.float32(par.usable_range)
    for r in c.frames:
        for k, (v, kept) in zip(ms.GATE_BEAMS, vals):
            assert bits(r[k : k + 1])[0] == bits([v])[0]
            x, _ = orc.clean_scan(r[k : k + 1], ang[k : k + 1], par.range_min, par.usable_range)
            assert len(x) == int(kept), f"beam {k} with range {v!r}"
    # the two equal values are kept; of the four neighbours the inner two are kept and the outer two dropped
    assert [kept for _, kept in vals] == [True, False, True, True, True, False, False, False]
    tr = trace(orc, "gate")
    assert tr[0]["scan_n"] == c.nbeams - 4


def test_crop_cases(orc):
    for s in ms.CROP_SIZES:
        tr = trace(orc, f"crop-size-{s}")
        assert tr[0]["map_n"] == s and tr[1]["rebuilt"] and tr[1]["map_before"] == s   # crop_kernel walks a map of exactly s
    # border 0: the points that span the scan's box lie ON it and the strict test drops them
    tr = trace(orc, "crop-border0")
    t = tr[1]
    assert t["rebuilt"] and 0 < t["lsize"] < t["map_before"]
    mx, my = tr[0]["map_x"], tr[0]["map_y"]
    dropped = ~t["keep"]
    extreme = (mx == mx.min()) | (mx == mx.max()) | (my == my.min()) | (my == my.max())
    assert dropped.any() and np.array_equal(dropped, extreme)
    # a later key frame from a moved pose: a proper subset, scattered across batches
    tr = trace(orc, "crop-moved")
    hit = []
    for f in range(2, len(tr)):
        t = tr[f]
        if not (t["rebuilt"] and tr[f - 1]["key"] and t["map_before"] > 1024 and 0 < t["lsize"] < t["map_before"]):
            continue
        idx = np.nonzero(t["keep"])[0]
        runs = 1 + int((np.diff(idx) > 1).sum())
        if runs >= 3 and (idx < 1024).any() and (idx >= 1024).any() and (~t["keep"])[:1024].any() and (~t["keep"])[1024:].any():
            hit.append(f)
    assert hit, "no rebuild after a key frame crops a scattered proper subset"


def test_raster_rooms_are_exactly_as_wide_as_the_storage(orc):
    tr = trace(orc, "raster-200")
    assert tr[1]["rebuilt"] and tr[1]["cols"][0] == 200 and tr[1]["cols"][1] <= 400 and max(tr[1]["rows"]) <= 200
    c = ms.case(orc, "raster-200")
    ang = c.angles(orc)
    x, y = orc.clean_scan(c.frames[0], ang)
    _, m = orc.rasterise(x, y, 0.2, 200)   # frame 1's local map is the whole first scan (checked next)
    assert tr[1]["lsize"] == tr[1]["map_before"] == len(x) and m.cols == 200
    # one column more: only its size is worked out here, the oracle is not run on it
    room = ms.raster_room(orc, 201)
    fits = ms.raster_room(orc, 200)
    assert 38.0 < fits[1] - fits[0] < room[1] - room[0] < 40.0
    assert round((room[1] - room[0] + 0.6) / 0.1) + 1 <= 400   # the fine grid still fits: the coarse guard alone trips


def test_empty_frame_is_no_key_frame(orc):
    c = ms.case(orc, "empty-frame")
    tr = trace(orc, "empty-frame")
    assert not c.frames[2].any() and tr[2]["scan_n"] == 0
    assert not tr[1]["key"] and not tr[2]["rebuilt"] and not tr[2]["key"]
    assert tr[2]["hits_n"] == 0
    assert all(t["scan_n"] == c.nbeams for f, t in enumerate(tr) if f != 2)


def test_append_cases(orc):
    tr = trace(orc, "append-grow")
    assert ms.case(orc, "append-grow").nbeams == 2049
    assert any(t["key"] and t["appended"] > 1024 for t in tr)
    assert any(t["key"] and t["appended"] == 0 for t in tr)
    # a hit that equals the threshold is not new
    c = ms.case(orc, "append-threshold")
    thr = np.float32(c.orc_params(orc).new_point_threshold)
    assert thr == np.float32(2.0)
    tr = trace(orc, "append-threshold")
    on = [t for t in tr if t["key"] and (t["hits"][: t["hits_n"]] == thr).any()]
    assert on
    for t in on:
        h = t["hits"][: t["hits_n"]]
        assert t["appended"] == t["candidates"] == int((h > thr).sum()) < int((h >= thr).sum())
    # the cap
    c = ms.case(orc, "append-cap")
    assert c.nbeams == 4096 and ms.MAP_CAP == 20000 + c.nbeams
    tr = trace(orc, "append-cap")
    full = [f for f, t in enumerate(tr) if t["map_n"] == ms.MAP_CAP]
    assert full and tr[-1]["map_n"] == ms.MAP_CAP
    assert any(t["key"] and t["candidates"] > t["appended"] > 0 for t in tr)   # the frame the clamp cuts short
    assert any(t["key"] and t["candidates"] > 0 and t["appended"] == 0 for t in tr[full[0] + 1 :])


def test_partial_case(orc):
    tr = trace(orc, "partial")
    frames = len(tr) - 1
    assert 2 * sum(t["partial"] for t in tr) >= frames
    assert any(t["partial"] and t["key"] and t["appended"] > 0 for t in tr)
    # several frames in a row match against a grid the scan outgrows
    assert any(tr[f]["partial"] and tr[f + 1]["partial"] and not tr[f + 1]["rebuilt"] for f in range(1, frames))


def test_restart_case_moves(orc):
    tr = trace(orc, "restart")
    assert len(tr) == 5 and any(t["key"] for t in tr) and bits(tr[-1]["pose"]).any()
