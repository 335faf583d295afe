"""slam_ekf_update_assoc_dev (the row update under a per-particle association table, csrc/assoc_kernels.hip) against
tests/_assoc_spec.py — orc_ekf_update with every particle's own observation list — bit for bit in the three forms; in place
nothing but the associated landmarks is touched; a table that is the same for every particle gives what slam_ekf_update_dev
gives for the equivalent observation table; the log-likelihoods stay in the engine."""
import numpy as np
import pytest
import torch

import _assoc_spec as A
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_aniso import make_case
from test_gpu_assoc import DEV, GATE, NEW_GATE, Q, detections, dev, eng, host   # noqa: F401 - eng is a fixture

pytestmark = pytest.mark.gpu
NS = (1, 3, 65, 1000)
LS = (1, 31, 128, 129, 257, 500)
FORMS = ("gather", "identity", "inplace")


def run_forms(eng, n, L, Lp, seed, K):
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, seed)
    anc = np.random.default_rng(seed + 1).integers(0, n, n).astype(np.int32)   # repeated and out-of-order ancestors
    dx, dy = detections(zx, zy, K, seed)
    eng.detections_upload(dx, dy)
    pose, d_in, d_ll = (dev(x), dev(y), dev(th)), dev(rows), torch.empty(n, device=DEV)
    for form in FORMS:
        label = f"n={n} L={L} Lp={Lp} {form}"
        a = anc if form == "gather" else None
        # the table of the spec for exactly these rows (junk in its padding columns: they are never read)
        assoc, st = A.associate(rows, x, y, th, a, dx, dy, Q, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
        assoc[:, L:] = np.arange(Lp - L, dtype=np.uint8)[None, :]
        want, want_ll = A.update(rows, x, y, th, a, assoc, dx, dy, Q, L=L, in_place=form == "inplace")
        d_assoc = dev(assoc)
        if form == "inplace":
            d_out = d_in.clone()
            eng.ekf_update_assoc_dev(d_out, d_out, 5 * Lp, Lp, L, *pose, None, n, Q, d_assoc, Lp, d_ll)
        else:
            d_out = torch.full((n, 5, Lp), 7.0, device=DEV)
            eng.ekf_update_assoc_dev(d_in, d_out, 5 * Lp, Lp, L, *pose, dev(a) if a is not None else None, n, Q, d_assoc, Lp, d_ll)
        got, got_ll = host(d_out), host(d_ll)
        assert np.array_equal(bits(got[:, :, :L]), bits(want[:, :, :L])), f"{label}: rows"
        assert np.array_equal(bits(got_ll), bits(want_ll)), f"{label}: log-likelihoods"
        if form == "inplace":   # nothing but the associated landmarks is touched, the padding included
            keep = np.ones((n, Lp), bool)
            keep[:, :L] = assoc[:, :L] == A.NONE
            keep = np.broadcast_to(keep[:, None, :], got.shape)
            assert np.array_equal(bits(got[keep]), bits(rows[keep])), f"{label}: columns without an association changed"
        if n >= 65 and L >= 31:
            assert st[:, 0].sum() > 0 and st[:, 1].sum() > 0
    assert np.array_equal(bits(host(d_in)), bits(rows)), "the source rows of an out-of-place update changed"


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_update_equals_the_spec(eng, n, L):
    run_forms(eng, n, L, (L + 31) // 32 * 32, 1000 * n + L, min(L, 40))


def test_plane_stride_a_multiple_of_128(eng):
    """... where whole batches run unpredicated over the padding (the fast path of the row walk)."""
    run_forms(eng, 65, 257, 384, 77, 64)


def test_a_uniform_table_is_the_known_correspondence_update(eng):
    """Every particle holds the same association: the result is slam_ekf_update_dev's for the observation table that says the
    same, on the GPU, bit for bit, in the three forms."""
    n, L, Lp, K = 65, 257, 288, 50
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, 21)
    rng = np.random.default_rng(2)
    ids = np.sort(rng.permutation(L)[:K]).astype(np.int32)      # landmark ids[j] ...
    k_of = rng.permutation(K)                                    # ... is detection k_of[j]
    dx, dy = np.empty(K, np.float32), np.empty(K, np.float32)
    dx[k_of], dy[k_of] = zx[ids], zy[ids]
    table = np.full((n, Lp), A.NONE, np.uint8)
    table[:, ids] = k_of
    anc = rng.integers(0, n, n).astype(np.int32)
    pose, d_in, d_table = (dev(x), dev(y), dev(th)), dev(rows), dev(table)
    eng.detections_upload(dx, dy)
    eng.obs_upload(ids, zx[ids], zy[ids], L)
    for form in FORMS:
        outs = []
        for assoc in (False, True):
            d_ll = torch.empty(n, device=DEV)
            d_out = d_in.clone() if form == "inplace" else torch.full((n, 5, Lp), 7.0, device=DEV)
            src = d_out if form == "inplace" else d_in
            d_anc = dev(anc) if form == "gather" else None
            if assoc:
                eng.ekf_update_assoc_dev(src, d_out, 5 * Lp, Lp, L, *pose, d_anc, n, Q, d_table, Lp, d_ll)
            else:
                eng.ekf_update_dev(src, d_out, 5 * Lp, Lp, L, *pose, d_anc, n, Q, d_ll)
            outs.append((host(d_out)[:, :, :L], host(d_ll)))
        assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1])), form


def test_loglikelihoods_stay_in_the_engine(eng):
    """slam_logweight_ekf_dev picks up what the update left: with a zero score, logw = loglik - 0."""
    n, L, Lp = 65, 31, 32
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, 9)
    dx, dy = detections(zx, zy, 20, 1)
    assoc, _ = A.associate(rows, x, y, th, None, dx, dy, Q, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
    _, want_ll = A.update(rows, x, y, th, None, assoc, dx, dy, Q, L=L)
    eng.detections_upload(dx, dy)
    d_out, logw, score = torch.empty((n, 5, Lp), device=DEV), torch.empty(n, device=DEV), torch.zeros(n, device=DEV)
    torch.cuda.synchronize()
    eng.ekf_update_assoc_dev(dev(rows), d_out, 5 * Lp, Lp, L, dev(x), dev(y), dev(th), None, n, Q, dev(assoc), Lp, None)
    eng.logweight_ekf_dev(score, 1.0, n, logw, None)
    eng.sync()
    assert np.any(want_ll != 0) and np.array_equal(bits(host(logw)), bits(want_ll - np.float32(0.0)))
