"""Rows, tables and evidence bytes that hold every branch of the merge rule (tests/_merge_spec.py) per particle.  TEST
INFRASTRUCTURE shared by test_merge_spec_cpu.py and test_gpu_merge.py; numpy only.

Anchor j of a particle sits at (4 j, i mod 3) — except j mod 4 == 3, which sits one metre to the right of anchor j - 1 with the
same covariance, so that the landmark half-way between them is at exactly the same cost from both.  The other slots take a kind
by (l + i) mod 12 and aim at anchor (l // 12 + i + GROUP[kind]) mod anchors: the kinds of one group contest one anchor."""
import numpy as np

F = np.float32
PERIOD = 12
ANCHOR_COV = ((0.5, 0.0, 0.5), (0.04, 0.03, 0.09), (0.5, 0.0, 0.5), (0.5, 0.0, 0.5), (0.3, -0.1, 0.2), (1.0, 1.0, 1.0), (2e-3, 0.0, 2e-3),
              (0.25, 0.0, 1.0))
KINDS = ("duplicate", "farther duplicate", "far away", "unseen", "NaN mean", "-0.0 in P_xx", "on the anchor", "on the anchor again",
         "singular S", "not positive definite", "a byte that names nothing", "between two anchors")
GROUP = (0, 0, 1, 1, 1, 1, 2, 2, 2, 3, 4, 5)


def anchor_at(i, j):
    if j % 4 == 3:
        x, y = anchor_at(i, j - 1)
        return x + 1.0, y
    return 4.0 * j, float(i % 3)


def make_case(n, L, plane_stride, K, anchors, seed):
    """-> (mp float32 [n][5][plane_stride], tab uint8 [n][L], c uint8 [n][L], kind int [n][L] (-1: an anchor)).  anchors: how many
    every particle gets (at most K and L); the padding columns and the unseen slots hold garbage and NaN."""
    rng = np.random.default_rng(seed)
    mp = (rng.standard_normal((n, 5, plane_stride)) * 1e3).astype(F)
    mp[rng.random(mp.shape) < 0.2] = np.nan
    tab = np.full((n, L), 255, np.uint8)
    c = rng.integers(0, 256, (n, L)).astype(np.uint8)
    kind = np.full((n, L), -1, np.int64)
    for i in range(n):
        na = min(anchors, K, L)
        slots = np.sort(rng.permutation(L)[:na])
        ks = rng.permutation(K)[:na]
        cov = {}
        for j, (l, k) in enumerate(zip(slots, ks)):
            cov[j] = ANCHOR_COV[(j - 1 if j % 4 == 3 else j) % len(ANCHOR_COV)]
            mp[i, :, l] = anchor_at(i, j) + cov[j]
            tab[i, l] = k
        for l in np.setdiff1d(np.arange(L), slots):
            kd = (l + i) % PERIOD
            kind[i, l] = kd
            t = (l // PERIOD + i + GROUP[kd]) % na if na else 0
            ax, ay = anchor_at(i, t)
            pw = cov[t] if na else ANCHOR_COV[0]
            x, y, p, byte = ax + 0.05, ay - 0.03, (0.05, 0.01, 0.04), 255
            if kd == 1:
                x, y = ax + 0.1, ay + 0.1
            elif kd == 2:
                y = ay + 500.0
            elif kd == 3:
                p = (-1.0, 0.0, 0.0)
            elif kd == 4:
                x = np.nan
            elif kd == 5:
                x, y, p = ax + 0.01, ay, (-0.0, 0.0, 0.04)
            elif kd in (6, 7):
                x, y, p = ax, ay, pw
            elif kd == 8:
                y, p = ay + 300.0, (1.0, 1.0, 1.0)
            elif kd == 9:
                x, y, p = ax, ay, (0.05, 0.2, 0.05)
            elif kd == 10:
                x, y, byte = ax + 0.02, ay + 0.02, min(K + 1, 254)
            elif kd == 11 and t - t % 4 + 3 < na:
                t = t - t % 4 + 2
                (x, y), p = anchor_at(i, t), (0.5, 0.0, 0.5)
                x = x + 0.5
            mp[i, :, l] = (x, y) + tuple(p)
            tab[i, l] = byte
    return mp, tab, c, kind
