"""slam_associate_detcov_dev and slam_ekf_update_assoc_detcov_dev (data association under a measurement covariance per detection,
csrc/assoc_kernels.hip: AssocNoiseDet, csrc/ekf_aniso_lane.h: EkfNoiseDet) against their specification
tests/_assoc_detcov_spec.py, bit for bit: the table's bytes over the whole stride and the stats, the rows and log-likelihoods of
the update in its three forms, a created landmark carrying R_w(i, k) of the detection that made it; the covariance hand-over, its
refusals and the counters."""
import numpy as np
import pytest
import torch

import _aniso_spec as S
import _assoc_aniso_spec as AA
import _assoc_detcov_spec as AD
import oracle
from _detections import covariances
from __graft_entry__ import load_package
from conftest import bits
from test_aniso_spec_cpu import q_matrix
from test_gpu_aniso import BAD, make_case
from test_gpu_assoc import DEV, GATE, NEW_GATE, detections, dev, eng, host   # noqa: F401 - eng is a fixture

pytestmark = pytest.mark.gpu
LS = (1, 31, 127, 128, 129, 257)     # one lane pair; the 128-landmark pass seam; the L <= 128 / L > 128 update instantiations
KS = (0, 1, 63, 64)
NS = (1, 5, 259)                     # no multiples of the waves per workgroup
FORMS = ("gather", "identity", "inplace")


def check(eng, poses, rows, L, dx, dy, covs, anc=None, stride=None, gate=GATE, new_gate=NEW_GATE, create=1, label=""):
    """One launch against the spec: table bytes (the whole stride) and stats; -> (table, stats)."""
    x, y, th = poses
    n, Lp = len(x), rows.shape[2]
    stride = L + 3 if stride is None else stride
    want, want_st = AD.associate(rows, x, y, th, anc, dx, dy, covs, gate, new_gate, create, L=L, assoc_stride=stride)
    d_rows = dev(rows)
    d_assoc = torch.full((n, stride), 7, dtype=torch.uint8, device=DEV)
    d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
    eng.detections_upload(dx, dy)
    eng.detections_cov_upload(*covs)
    eng.associate_detcov_dev(d_rows, 5 * Lp, Lp, L, dev(x), dev(y), dev(th), dev(anc) if anc is not None else None, n, gate, new_gate,
                             create, d_assoc, stride, d_st)
    got, got_st = host(d_assoc), host(d_st)
    assert np.array_equal(got, want), f"{label}: table differs at {np.argwhere(got != want)[:5].tolist()}"
    assert np.array_equal(got_st, want_st), f"{label}: stats"
    assert np.array_equal(bits(host(d_rows)), bits(rows)), f"{label}: the source rows changed"
    return want, want_st


def update_forms(eng, poses, rows, L, dx, dy, covs, anc, label):
    """The update in its three forms against the spec, under the spec's own table for exactly these rows."""
    x, y, th = poses
    n, Lp = len(x), rows.shape[2]
    pose, d_in, d_ll = (dev(x), dev(y), dev(th)), dev(rows), torch.empty(n, device=DEV)
    eng.detections_upload(dx, dy)
    eng.detections_cov_upload(*covs)
    s, c = oracle.det_sincos(th)
    ncreated = 0
    for form in FORMS:
        a = anc if form == "gather" else None
        assoc, st = AD.associate(rows, x, y, th, a, dx, dy, covs, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
        assoc[:, L:] = np.arange(Lp - L, dtype=np.uint8)[None, :]     # junk in the table's padding columns: they are never read
        want, want_ll = AD.update(rows, x, y, th, a, assoc, dx, dy, covs, L=L, in_place=form == "inplace")
        d_assoc = dev(assoc)
        if form == "inplace":
            d_out = d_in.clone()
            eng.ekf_update_assoc_detcov_dev(d_out, d_out, 5 * Lp, Lp, L, *pose, None, n, d_assoc, Lp, d_ll)
        else:
            d_out = torch.full((n, 5, Lp), 7.0, device=DEV)
            eng.ekf_update_assoc_detcov_dev(d_in, d_out, 5 * Lp, Lp, L, *pose, dev(a) if a is not None else None, n, d_assoc, Lp, d_ll)
        got, got_ll = host(d_out), host(d_ll)
        assert np.array_equal(bits(got[:, :, :L]), bits(want[:, :, :L])), f"{label} {form}: rows"
        assert np.array_equal(bits(got_ll), bits(want_ll)), f"{label} {form}: log-likelihoods"
        src = np.arange(n) if a is None else a
        created = (rows[src][:, 2, :L] < 0) & (assoc[:, :L] < len(dx))
        ncreated += int(created.sum())
        if created.any():   # a created landmark carries R_w(theta_i, k) of the detection that made it
            ii, ll_ = np.nonzero(created)
            k = assoc[ii, ll_].astype(np.int64)
            rw = S.world_noise((covs[0][k], covs[1][k], covs[2][k]), s[ii], c[ii])
            for j in range(3):
                assert np.array_equal(bits(got[ii, 2 + j, ll_]), bits(rw[j])), f"{label} {form}: R_w of a created landmark"
        if form == "inplace":   # nothing but the associated landmarks is touched, the padding included
            keep = np.ones((n, Lp), bool)
            keep[:, :L] = assoc[:, :L] >= len(dx)
            keep = np.broadcast_to(keep[:, None, :], got.shape)
            assert np.array_equal(bits(got[keep]), bits(rows[keep])), f"{label}: columns without an association changed"
    assert np.array_equal(bits(host(d_in)), bits(rows)), "the source rows of an out-of-place update changed"
    return ncreated


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_table_and_update_equal_the_spec(eng, n, L):
    """Every K with every Q_k different, create 0 and 1, with and without a gather index of repeated, out-of-order ancestors;
    plane_stride and assoc_stride leave padding columns (every other K: a stride that is no multiple of 4)."""
    Lp = (L + 32) // 32 * 32                                           # > L
    poses, rows, zx, zy = make_case(n, L, Lp, 1000 * n + L)
    anc = np.random.default_rng(n + L).integers(0, n, n).astype(np.int32)
    matched = created = dropped = 0
    for j, K in enumerate(KS):
        dx, dy = detections(zx, zy, K, K)
        covs = covariances(K, 100 * L + K)
        for a in (None, anc):
            for create in (1, 0):
                _, st = check(eng, poses, rows, L, dx, dy, covs, anc=a, stride=Lp if j % 2 == 0 else L + 3, create=create,
                              label=f"n={n} L={L} K={K} anc={a is not None} create={create}")
                matched += int(st[:, 0].sum())
                created += int(st[:, 1].sum())
                dropped += int(st[:, 2].sum()) if create else 0
        update_forms(eng, poses, rows, L, dx, dy, covs, anc, f"n={n} L={L} K={K}")
    if L <= 31:
        assert dropped > 0                                             # (more detections that belong to nothing than unseen slots)
    if n >= 5 and L >= 31:
        assert matched > 0 and created > 0


def test_update_with_a_plane_stride_a_multiple_of_128(eng):
    """... where whole batches run unpredicated over the padding (the fast path of the row walk), two batches per pass."""
    n, L, Lp = 67, 300, 512
    poses, rows, zx, zy = make_case(n, L, Lp, 77)
    dx, dy = detections(zx, zy, 64, 3)
    anc = np.random.default_rng(8).integers(0, n, n).astype(np.int32)
    assert update_forms(eng, poses, rows, L, dx, dy, covariances(64, 9), anc, "Lp=512") > 0


def test_unseen_slots_run_out(eng):
    n, L, Lp = 5, 20, 32
    poses, rows, zx, zy = make_case(n, L, Lp, 12)
    dx, dy = detections(zx, zy, 33, 5)
    covs = covariances(33, 6)
    unseen = rows.copy()
    unseen[:, 2, :L] = -1.0
    _, st = check(eng, poses, unseen, L, dx, dy, covs, stride=32, label="all unseen, slots run out")
    assert np.all(st == [0, 20, 13])
    update_forms(eng, poses, unseen, L, dx, dy, covs, np.array([4, 4, 0, 1, 1], np.int32), "all unseen")
    seen = rows.copy()
    seen[:, 2, :L] = np.abs(seen[:, 2, :L])
    _, st = check(eng, poses, seen, L, dx, dy, covs, label="none unseen")
    assert np.all(st[:, 1] == 0) and st[:, 2].sum() > 0


def test_duplicate_detections_and_the_same_point_under_two_covariances(eng):
    n, L, Lp = 65, 129, 160
    poses, rows, zx, zy = make_case(n, L, Lp, 11)
    rows[:, 2, :L] = np.abs(rows[:, 2, :L])                            # everything seen
    dx, dy = detections(zx, zy, 20, 3)
    dx[:3], dy[:3] = zx[[5, 66, 9]], zy[[5, 66, 9]]
    qxx, qxy, qyy = covariances(20, 4)
    # the same z and the same Q twice: the landmark takes the lower k, the copy is never chosen
    dx[7], dy[7] = dx[2], dy[2]
    qxx[7], qxy[7], qyy[7] = qxx[2], qxy[2], qyy[2]
    # the same z under two covariances, the second ten times tighter: whichever the spec says, per particle
    dx[11], dy[11] = dx[0], dy[0]
    qxx[11], qxy[11], qyy[11] = (np.float32(0.1) * v for v in (qxx[0], qxy[0], qyy[0]))
    want, st = check(eng, poses, rows, L, dx, dy, (qxx, qxy, qyy), label="duplicates")
    assert st[:, 0].sum() > 0 and not np.any(want == 7)
    update_forms(eng, poses, rows, L, dx, dy, (qxx, qxy, qyy), np.arange(n, dtype=np.int32)[::-1].copy(), "duplicates")


def test_headings_through_plus_and_minus_pi(eng):
    n, L, Lp = 9, 40, 64
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, 21)
    pi = np.float32(np.pi)
    th[:8] = [pi, -pi, np.nextafter(pi, np.float32(4)), np.nextafter(-pi, np.float32(-4)), np.nextafter(pi, np.float32(0)),
              np.nextafter(-pi, np.float32(0)), 3 * pi, -3 * pi]
    dx, dy = detections(zx, zy, 40, 2)
    covs = covariances(40, 3)
    check(eng, (x, y, th), rows, L, dx, dy, covs, label="headings")
    update_forms(eng, (x, y, th), rows, L, dx, dy, covs, np.random.default_rng(2).integers(0, n, n).astype(np.int32), "headings")


def test_all_covariances_equal_is_the_aniso_stage(eng):
    """Every Q_k the same Q: the bytes, rows and log-likelihoods of slam_associate_aniso_dev / slam_ekf_update_assoc_aniso_dev."""
    n, L, Lp = 67, 129, 160
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, 31)
    dx, dy = detections(zx, zy, 64, 4)
    cov = (np.float32(0.02), np.float32(0.012), np.float32(0.015))
    covs = tuple(np.full(64, v, np.float32) for v in cov)
    want, _ = check(eng, (x, y, th), rows, L, dx, dy, covs, stride=Lp, label="all equal")
    ref, _ = AA.associate(rows, x, y, th, None, dx, dy, cov, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
    assert np.array_equal(want, ref)
    d_in, d_a, d_b, d_ll = dev(rows), torch.full((n, 5, Lp), 7.0, device=DEV), torch.full((n, 5, Lp), 7.0, device=DEV), torch.empty(n, device=DEV)
    args = (5 * Lp, Lp, L, dev(x), dev(y), dev(th), None, n)
    eng.ekf_update_assoc_detcov_dev(d_in, d_a, *args, dev(want), Lp, d_ll)
    ll_a = host(d_ll).copy()
    eng.ekf_update_assoc_aniso_dev(d_in, d_b, *args, cov, dev(want), Lp, d_ll)
    assert np.array_equal(bits(host(d_a)[:, :, :L]), bits(host(d_b)[:, :, :L])) and np.array_equal(bits(ll_a), bits(host(d_ll)))


def test_hand_over_refusals_and_counters(eng):
    pkg = load_package()
    n, L, Lp = 3, 31, 32
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, 3)
    d_rows, d_assoc = dev(rows), torch.full((n, Lp), 7, dtype=torch.uint8, device=DEV)
    d_out = torch.full((n, 5, Lp), 7.0, device=DEV)
    pose = (dev(x), dev(y), dev(th))
    assoc_call = lambda e: e.associate_detcov_dev(d_rows, 5 * Lp, Lp, L, *pose, None, n, GATE, NEW_GATE, 1, d_assoc, Lp, None)
    update_call = lambda e: e.ekf_update_assoc_detcov_dev(d_rows, d_out, 5 * Lp, Lp, L, *pose, None, n, d_assoc, Lp, None)

    def refused(call, status):
        with pytest.raises(pkg.SlamError) as err:
            call()
        assert err.value.status == status, str(err.value)

    fresh = pkg.Engine(0)
    one = np.ones(5, np.float32)
    refused(lambda: fresh.detections_cov_upload(one, 0 * one, one), -4)          # no detections at all
    refused(lambda: fresh.detections_cov(), -4)
    refused(lambda: assoc_call(fresh), -4)
    fresh.close()

    counters = lambda: (eng.assoc_detcov_counts(), eng.assoc_aniso_counts(), eng.assoc_counts(), eng.ekf_aniso_count(), eng.ekf_form_counts(),
                        eng.ekf_inplace_form_counts())
    eng.detections_upload(zx[:5], zy[:5])
    c0 = counters()
    for call in (assoc_call, update_call):                                        # detections without covariances
        refused(lambda: call(eng), -4)
    refused(lambda: eng.detections_cov(), -4)
    good = covariances(5, 1)
    refused(lambda: eng.detections_cov_upload(*(v[:4] for v in good)), -2)        # a mismatched ndet
    refused(lambda: eng.detections_cov_upload(*(np.append(v, v[0]) for v in good)), -2)
    refused(lambda: assoc_call(eng), -4)                                          # ... changed nothing
    eng.detections_cov_upload(*good)
    for q in BAD:                                                                 # a bad Q_k, in any place, changes nothing
        for k in (0, 4):
            bad = [v.copy() for v in good]
            for j in range(3):
                bad[j][k] = q[j]
            refused(lambda: eng.detections_cov_upload(*bad), -2)
    back = eng.detections_cov()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(back, good))
    ok = dict(gate=GATE, new_gate=NEW_GATE, create=1, L=L, stride=Lp)
    for change in (dict(gate=0.0), dict(gate=float("nan")), dict(gate=float("inf")), dict(new_gate=GATE / 2), dict(L=8193, stride=8193),
                   dict(stride=L - 1), dict(create=2)):
        a = dict(ok, **change)
        refused(lambda: eng.associate_detcov_dev(d_rows, 5 * max(Lp, a["L"]), max(Lp, a["L"]), a["L"], *pose, None, n, a["gate"],
                                                 a["new_gate"], a["create"], d_assoc, a["stride"], None), -2)
    d_anc = dev(np.zeros(n, np.int32))
    refused(lambda: eng.ekf_update_assoc_detcov_dev(d_rows, d_rows, 5 * Lp, Lp, L, *pose, d_anc, n, d_assoc, Lp, None), -2)   # gather in place
    refused(lambda: eng.ekf_update_assoc_detcov_dev(d_rows, d_out, 5 * Lp, Lp, L, *pose, None, n, d_assoc, L - 1, None), -2)
    assert counters() == c0 and np.all(host(d_assoc) == 7) and np.all(host(d_out) == 7.0)   # nothing was launched
    assoc_call(eng)
    update_call(eng)
    eng.sync()
    c1 = counters()
    assert c1[0] == (c0[0][0] + 1, c0[0][1] + 1) and c1[1:] == c0[1:]             # the new counter alone
    want, _ = AD.associate(rows, x, y, th, None, zx[:5], zy[:5], good, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
    assert np.array_equal(host(d_assoc), want)
    # the device form adopts its arrays
    d_q = [dev(v) for v in good]
    eng.detections_cov_set_dev(*d_q, 5)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(eng.detections_cov(), good))
    refused(lambda: eng.detections_cov_set_dev(*d_q, 4), -2)
    # new detections carry no covariance
    eng.detections_upload(zx[:5], zy[:5])
    refused(lambda: eng.detections_cov(), -4)
    refused(lambda: assoc_call(eng), -4)
    refused(lambda: update_call(eng), -4)
    eng.detections_cov_upload(*good)
    d_z = (dev(zx[:5]), dev(zy[:5]))
    eng.detections_set_dev(*d_z, 5)
    refused(lambda: assoc_call(eng), -4)
    assert counters() == c1
