"""Every path a slam_pf frame can take, against one rank on rows, bit for bit.

Five map layouts x {one GPU, three ranks sharing this card} x {ungated, ESS-gated} x {dense, sparse observations}: which
launches a frame consists of is decided by the host code of csrc/pf_session_frame.hip from exactly these four facts.  At 9 216
particles x 160 landmarks (3 072 per rank of three, rows of five pages) the fused front (one GPU and sharded), the staging
tail, the free-list rider, both forms of the paged update, the gathers of the frame without observations and the exchange
that a map read completes early all occur.  Results never depend on the layout, the number of ranks or the path taken.

No combination is refused at session creation: all 40 run.
"""
import numpy as np
import pytest

from conftest import bits
from test_gpu_configs import _run_c_session_ranks

pytestmark = pytest.mark.gpu

N_TOTAL, L, FRAMES = 9216, 160, 8
_reference_runs = {}


def _reference(ess, sparse_obs):
    """One rank on rows, once per (ess, sparse_obs); nobody writes to what it returns."""
    key = (ess, sparse_obs)
    if key not in _reference_runs:
        _reference_runs[key] = _run_c_session_ranks(1, N_TOTAL, L, FRAMES, transport=None, layout="rows", ess=ess,
                                                    sparse_obs=sparse_obs, maps_every_frame=True)[0]
    return _reference_runs[key]


@pytest.mark.parametrize("sparse_obs", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("ess", [0.0, 0.4], ids=["ungated", "gated"])
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("layout", ["rows", "split", "pages", "split_pages", "auto"])
def test_session_paths_give_the_bits_of_one_rank_on_rows(layout, world, ess, sparse_obs):
    ref = _reference(ess, sparse_obs)
    ranks = _run_c_session_ranks(world, N_TOTAL, L, FRAMES, transport=None if world == 1 else "local", layout=layout, ess=ess,
                                 sparse_obs=sparse_obs, maps_every_frame=True)
    assert np.array_equal(bits(np.concatenate([p["pose"] for p in ranks], axis=1)), bits(ref["pose"]))
    assert np.array_equal(bits(np.concatenate([p["map"] for p in ranks], axis=0)), bits(ref["map"]))
    for f in range(FRAMES):
        got = np.concatenate([p["frame_maps"][f] for p in ranks], axis=0)
        assert np.array_equal(bits(got), bits(ref["frame_maps"][f])), f
    for p in ranks:
        assert p["best"][2] == ref["best"][2] and np.array_equal(bits(p["best"][1]), bits(ref["best"][1]))
        assert np.array_equal(bits(p["best"][0]), bits(ref["best"][0]))
        assert np.array_equal(bits(p["mean"]), bits(ref["mean"]))
    # what can be seen of the path taken
    if ess == 0.0 and (layout == "split" or (layout == "rows" and world == 1)):
        assert all(p["fused"] > 0 for p in ranks), [p["fused"] for p in ranks]
    if layout != "auto":
        assert all(set(p["layouts"]) == {layout} for p in ranks), [p["layouts"] for p in ranks]
    if world == 3:
        assert sum(sum(p["rows"]) for p in ranks) > 0, "nothing migrated"
