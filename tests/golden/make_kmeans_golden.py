"""Generate tests/golden/kmeans.npz and tests/golden/kmeans_signatures.json.

    python tests/golden/make_kmeans_golden.py

The signature comes from the REAL reference (TorchDR at /root/reference; its eval module imports without faiss).  The
reference's own k-means needs faiss and torchmetrics, so the values come from an independent code, scikit-learn:

* ``ari_pred_<i>`` / ``ari_true_<i>`` / ``ari_score``: label pairs and ``adjusted_rand_score`` in float64, plus
  ``ari_big_score`` for the N = 300k pair that ``big_pair()`` rebuilds (past the int64 overflow of pair-count products).
* ``lloyd_<name>_{X,init,labels,inertia,niter}``: small datasets, fixed initial centres, and ``KMeans(init=init,
  n_init=1, max_iter=niter, tol=0, algorithm="lloyd")``'s labels and inertia.  No cluster empties and N <= 256 * C.
* ``quality_<name>``: ``adjusted_rand_score`` of ``KMeans(init="random", n_init=1, max_iter=20, random_state=s)`` for
  s = 0..19 on ``mixture(name)`` (tests.conftest.gmm, rebuilt from a seeded CPU torch.Generator; only scores are stored).

The npz is written with fixed zip timestamps, so a second run reproduces the same bytes.
"""

import inspect
import io
import json
import os
import sys
import warnings
import zipfile

os.environ["OMP_NUM_THREADS"] = "1"   # sklearn's threaded inertia sum is not reproducible to the last bit

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

from sklearn.cluster import KMeans  # noqa: E402
from sklearn.metrics import adjusted_rand_score  # noqa: E402
from torchdr.eval.kmeans import kmeans_ari  # noqa: E402


def save_npz(path, arrs):
    """np.savez_compressed with a fixed timestamp per member (reproducible bytes)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrs[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def big_pair():
    """N = 300k, 10 classes; pred = true with 30 % of the entries redrawn."""
    g = np.random.default_rng(300_000)
    true = g.integers(0, 10, 300_000)
    pred = true.copy()
    flip = g.random(300_000) < 0.3
    pred[flip] = g.integers(0, 10, int(flip.sum()))
    return pred.astype(np.int64), true.astype(np.int64)


def mixture(name):
    """The quality-band mixtures: tests.conftest.gmm(20000, 64, scale) with its 200 groups (labels arange(n) % 200)."""
    n, d = 20000, 64
    scale = {"separated": 2.0, "overlapping": 0.5}[name]
    g = torch.Generator().manual_seed(42)
    nc = 200
    centers = torch.randn(nc, d, generator=g) * scale
    labels = torch.arange(n) % nc
    return (centers[labels] + 0.5 * torch.randn(n, d, generator=g)).contiguous(), labels


QUALITY_SEEDS = 20   # the spread of one run's ARI is ~0.05 here: a band from 5 seeds would move by ~0.02 with the seeds


def ari_pairs():
    g = np.random.default_rng(20261016)
    pairs = []
    a = g.integers(0, 5, 40)
    pairs += [
        (np.zeros(10, np.int64), np.zeros(10, np.int64)),            # all one label
        (np.arange(10), np.arange(10)),                              # all distinct
        (np.arange(10), np.zeros(10, np.int64)),                     # distinct vs one
        (np.zeros(10, np.int64), np.arange(10)),
        (np.array([3]), np.array([-1])),                             # N = 1
        (np.array([0, 1]), np.array([5, 5])),                        # N = 2
        (np.array([0, 0]), np.array([1, 2])),
        (np.array([4, 4]), np.array([9, 9])),
        (a, (a + 2) % 5),                                            # permuted labels: 1.0
        (a, np.array([-7, 10**12, 3, -(10**15), 0])[a]),              # negative and very large ids, permuted: 1.0
        (a, np.where(np.arange(40) == 17, (a + 1) % 5, a)),          # a single mismatch
    ]
    for n, k1, k2 in [(50, 3, 3), (100, 2, 7), (200, 10, 10), (500, 4, 20), (1000, 50, 3), (33, 33, 2)]:
        pairs.append((g.integers(0, k1, n), g.integers(0, k2, n)))
    for n, k, p in [(300, 5, 0.1), (1000, 8, 0.5), (2000, 20, 0.2), (5000, 3, 0.9), (400, 40, 0.3)]:
        t = g.integers(0, k, n)
        q = t.copy()
        f = g.random(n) < p
        q[f] = g.integers(0, k, int(f.sum()))
        pairs.append((q, t))
    for n in (3, 4, 6, 8):
        pairs.append((g.integers(-3, 3, n), g.integers(100, 102, n)))
    pairs.append((np.repeat(np.arange(4), 25), np.tile(np.arange(4), 25)))   # orthogonal partitions
    pairs.append((np.repeat(np.arange(2), 50), np.repeat(np.arange(4), 25)))  # nested partitions
    return [(np.asarray(p, np.int64), np.asarray(t, np.int64)) for p, t in pairs]


def no_empty_cluster(X, C, niter):
    """Plain Lloyd in float64 (sklearn relocates empty clusters, faiss splits them: the fixture avoids both)."""
    X, C = X.astype(np.float64), C.astype(np.float64)
    for _ in range(niter):
        lab = ((X[:, None, :] - C[None]) ** 2).sum(-1).argmin(1)
        cnt = np.bincount(lab, minlength=len(C))
        if cnt.min() == 0:
            return False
        C = np.stack([X[lab == k].mean(0) for k in range(len(C))])
    return True


def lloyd_sets():
    g = np.random.default_rng(7)
    out = {}
    for name, n, d, C, niter, spread in [("d2", 600, 2, 4, 10, 1.2), ("d16", 1000, 16, 8, 10, 1.5), ("d264", 300, 264, 5, 8, 0.3)]:
        cen = g.normal(size=(C, d)) * 2.0
        lab = np.arange(n) % C
        X = (cen[lab] + spread * g.normal(size=(n, d))).astype(np.float32)
        init = X[g.choice(n // C, C) * C + np.arange(C)].copy()      # one row of every group
        assert no_empty_cluster(X, init, niter), name
        km = KMeans(n_clusters=C, init=init.astype(np.float64), n_init=1, max_iter=niter, tol=0, algorithm="lloyd")
        km.fit(X.astype(np.float64))
        assert np.bincount(km.labels_, minlength=C).min() > 0
        out[name] = dict(X=X, init=init, labels=km.labels_.astype(np.int64), inertia=np.float64(km.inertia_),
                         niter=np.int64(niter))
    return out


def main():
    torch.set_num_threads(4)
    out = {}
    pairs = ari_pairs()
    scores = []
    for i, (p, t) in enumerate(pairs):
        out[f"ari_pred_{i}"] = p
        out[f"ari_true_{i}"] = t
        scores.append(adjusted_rand_score(t, p))
    out["ari_score"] = np.array(scores, np.float64)
    bp, bt = big_pair()
    out["ari_big_score"] = np.float64(adjusted_rand_score(bt, bp))
    for name, v in lloyd_sets().items():
        for k, a in v.items():
            out[f"lloyd_{name}_{k}"] = a
    for name in ("separated", "overlapping"):
        X, lab = mixture(name)
        s = []
        for seed in range(QUALITY_SEEDS):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                km = KMeans(n_clusters=200, init="random", n_init=1, max_iter=20, random_state=seed).fit(X.numpy())
            s.append(adjusted_rand_score(lab.numpy(), km.labels_))
        out[f"quality_{name}"] = np.array(s, np.float64)
        print(name, np.round(s, 4))
    path = os.path.join(HERE, "kmeans.npz")
    save_npz(path, out)
    print(f"kmeans: {os.path.getsize(path) / 1024:.0f} KiB, {len(pairs)} ARI pairs, big {out['ari_big_score']:.6f}")

    ps = inspect.signature(kmeans_ari).parameters
    sigs = {"eval.kmeans_ari": [[k, None if v.default is inspect._empty else repr(v.default)] for k, v in ps.items()]}
    with open(os.path.join(HERE, "kmeans_signatures.json"), "w") as f:
        json.dump(sigs, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
