"""kmeans_ari on the HIP k-means kernels: the reference's test shapes, the assignment kernel against the exact k = 1 search
(bit for bit), one Lloyd step and the empty-cluster split against float64 / host restatements, whole runs against
scikit-learn's recorded Lloyd runs (tests/golden/kmeans.npz), the documented training subsample, ARI on the device
path, a quality band and one 1M-row run."""

import os
import time

import numpy as np
import pytest
import torch

from tests.conftest import gmm, grade64

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
M64 = (1 << 64) - 1


def _golden():
    return np.load(os.path.join(HERE, "golden", "kmeans.npz"))


def _K():
    from torchdr_amd.eval import kmeans as K

    return K


# ---- the reference's test shapes (torchdr/tests/test_eval.py:190-357), on this package's own data ----------------------

def _blobs(n_per=50, seed=42):
    g = np.random.default_rng(seed)
    X = np.vstack([g.normal(size=(n_per, 2)) + np.array(c) for c in ([0, 0], [10, 10], [-10, 10])]).astype("float32")
    return X, np.repeat(np.arange(3), n_per)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_basic_return_types(dtype):
    from torchdr_amd import kmeans_ari

    g = np.random.default_rng(0)
    X = g.normal(size=(100, 10)).astype(dtype)
    y = g.integers(0, 3, 100)
    s, lab = kmeans_ari(X, y, random_state=0)
    assert isinstance(s, float) and -1 <= s <= 1
    assert isinstance(lab, np.ndarray) and lab.shape == (100,) and lab.dtype == np.int64
    st, labt = kmeans_ari(torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV), random_state=0)
    assert isinstance(st, torch.Tensor) and st.dim() == 0 and st.dtype == torch.float32 and st.device.type == "cuda"
    assert isinstance(labt, torch.Tensor) and labt.dtype == torch.int64 and labt.shape == (100,) and labt.device.type == "cuda"
    assert float(st) == np.float32(s) and np.array_equal(labt.cpu().numpy(), lab)
    # CPU tensors: computed on the HIP device, returned on X's device; an explicit device wins
    sc, labc = kmeans_ari(torch.from_numpy(X), torch.from_numpy(y), random_state=0)
    assert sc.device.type == "cpu" and labc.device.type == "cpu"
    sd, labd = kmeans_ari(torch.from_numpy(X), torch.from_numpy(y), random_state=0, device="cuda")
    assert sd.device.type == "cuda" and labd.device.type == "cuda"
    # mixed input (one tensor, one array): the numpy form
    sm, labm = kmeans_ari(torch.from_numpy(X).to(DEV), y, random_state=0)
    assert isinstance(sm, float) and isinstance(labm, np.ndarray)


def test_n_clusters():
    from torchdr_amd import kmeans_ari

    X, y = _blobs()
    s_auto, lab_auto = kmeans_ari(X, y, random_state=1)
    s3, lab3 = kmeans_ari(X, y, n_clusters=3, random_state=1)
    assert s_auto == s3 and np.array_equal(lab_auto, lab3)
    _, lab4 = kmeans_ari(X, y, n_clusters=4, random_state=1)
    assert len(np.unique(lab4)) <= 4
    # labels of any integer values: negative, non-contiguous, a trailing unit dimension
    s_neg, lab_neg = kmeans_ari(X, (np.array([-5, 7, 1000])[y])[:, None], random_state=1)
    assert s_neg == s3 and np.array_equal(lab_neg, lab3)


def test_reproducibility():
    from torchdr_amd import kmeans_ari

    g = np.random.default_rng(3)
    X = g.normal(size=(400, 6)).astype("float32")
    y = g.integers(0, 5, 400)
    s1, l1 = kmeans_ari(X, y, random_state=42)
    s2, l2 = kmeans_ari(X, y, random_state=42)
    assert s1 == s2 and np.array_equal(l1, l2)
    _, l3 = kmeans_ari(X, y, random_state=123)
    assert not np.array_equal(l1, l3)


def test_perfect_clustering():
    from torchdr_amd import kmeans_ari

    X, y = _blobs()
    s, lab = kmeans_ari(X, y, n_clusters=3, nredo=5)
    assert s == 1.0
    assert len(np.unique(lab)) == 3


def test_niter_nredo_and_edge_cases():
    from torchdr_amd import kmeans_ari

    g = np.random.default_rng(5)
    X = g.normal(size=(100, 5)).astype("float32")
    y = g.integers(0, 2, 100)
    for kw in (dict(niter=5), dict(niter=50), dict(nredo=1), dict(nredo=5), dict(niter=0)):
        s, lab = kmeans_ari(X, y, n_clusters=2, random_state=42, **kw)
        assert -1 <= s <= 1 and lab.shape == (100,) and lab.min() >= 0 and lab.max() < 2
    X5 = g.normal(size=(5, 3)).astype("float32")
    s, lab = kmeans_ari(X5, np.arange(5), n_clusters=5, random_state=0)
    assert -1 <= s <= 1 and len(lab) == 5
    X4 = np.array([[0, 0], [0, 1], [10, 10], [10, 11]], dtype="float32")
    s, lab = kmeans_ari(X4, np.array([0, 0, 1, 1]), n_clusters=2, random_state=0)
    assert s > 0.5 and len(lab) == 4


def test_verbose_prints(capsys):
    from torchdr_amd import kmeans_ari

    X, y = _blobs()
    kmeans_ari(X, y, niter=3, random_state=0, verbose=True)
    out = capsys.readouterr().out
    assert out.count("objective") == 3


# ---- assignment kernel == exact k = 1 search, bit for bit ---------------------------------------------------------------

def _knn1(X, C):
    from torchdr_amd.distance.base import PackedPoints, _knn_wide, knn_packed

    if X.shape[1] > 256:
        return _knn_wide(X, C, 1, "sqeuclidean", False)
    return knn_packed(PackedPoints(X), PackedPoints(C), 1, "sqeuclidean", False)


@pytest.mark.parametrize("d", [1, 2, 3, 50, 128, 256, 257, 784, 1500])
@pytest.mark.parametrize("c", [1, 2, 7, 64, 1000, 4096, "N"])
def test_assign_equals_knn_k1(d, c):
    K = _K()
    n = 5000
    g = torch.Generator().manual_seed(1000 * d + (0 if c == "N" else c))
    base = torch.round(torch.randn(n // 2, d, generator=g) * 4) / 4     # quantised: equal distances occur
    X = base[torch.randint(0, n // 2, (n,), generator=g)].to(DEV)       # exact duplicate rows
    c = n if c == "N" else c
    C = X[:c].contiguous()                                               # duplicate centres: ties by index
    labels, dist, obj = K.assign(K.pack(X), n, C)
    ref_d, ref_i = _knn1(X, C)
    assert torch.equal(labels, ref_i[:, 0])
    assert torch.equal(dist.view(torch.int32), ref_d[:, 0].contiguous().view(torch.int32))
    ref_obj = dist.double().sum().item()
    assert abs(obj.item() - ref_obj) <= 1e-9 * max(abs(ref_obj), 1e-30)
    labels2, dist2, obj2 = K.assign(K.pack(X), n, C)
    assert torch.equal(labels, labels2) and torch.equal(dist, dist2) and obj.item() == obj2.item()


# ---- one Lloyd step against a float64 restatement ------------------------------------------------------------------------

@pytest.mark.parametrize("d", [32, 300])
@pytest.mark.parametrize("c", [3, 100, 2000])
def test_one_step_graded(d, c):
    K = _K()
    n = 20000
    g = torch.Generator().manual_seed(d + c)
    X = torch.randn(n, d, generator=g).to(DEV)
    C0 = X[:c].contiguous()
    labels, dist, obj = K.assign(K.pack(X), n, C0)
    C = C0.clone()
    counts, perm = K.update(X, labels, C)
    lab64 = labels.long()
    ref_counts = torch.bincount(lab64, minlength=c)
    assert torch.equal(counts.long(), ref_counts)
    assert torch.equal(perm.long(), torch.argsort(lab64, stable=True))
    assert int(ref_counts.min()) > 0
    sums = torch.zeros(c, d, dtype=torch.float64, device=DEV).index_add_(0, lab64, X.double())
    grade64(f"kmeans_step_centres_{d}_{c}", C, sums / ref_counts[:, None].double(), 1e-6)
    ref_obj = dist.double().sum().item()
    assert abs(obj.item() - ref_obj) <= 1e-6 * abs(ref_obj)
    C2 = C0.clone()
    K.update(X, labels, C2)
    assert torch.equal(C.view(torch.int32), C2.view(torch.int32))


# ---- empty clusters: faiss's split, restated on the host -----------------------------------------------------------------

def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _split_ref(cent, cnt, seed, it):
    cent = cent.copy()
    cnt = list(cnt)
    up, down = np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)
    hosts = {}
    for ci in range(len(cnt)):
        if cnt[ci] != 0:
            continue
        total = sum(max(x - 1, 0) for x in cnt)
        if total == 0:
            continue
        u = _splitmix64(seed ^ _splitmix64(((it & 0xFFFFFFFF) << 32) | ci)) % total
        run = 0
        for cj in range(len(cnt)):
            run += max(cnt[cj] - 1, 0)
            if run > u:
                break
        v = cent[cj].copy()
        even = (np.arange(v.size) % 2) == 0
        cent[ci] = np.where(even, v * up, v * down)
        cent[cj] = np.where(even, v * down, v * up)
        half = cnt[cj] // 2
        cnt[ci] = half
        cnt[cj] -= half
        hosts[ci] = cj
    return cent, cnt, hosts


def _dup_data():
    g = torch.Generator().manual_seed(11)
    P = torch.randn(50, 8, generator=g)
    X = P[torch.arange(1000) % 50].contiguous()         # every point 20 times; rows i and i + 50 are equal
    init_rows = torch.tensor([0, 50, 1, 51, 2, 100, 3, 4, 150, 5])   # centres 1, 3, 5, 8 duplicate lower ones
    return X.to(DEV), X[init_rows].contiguous().to(DEV)


def test_empty_cluster_split():
    K = _K()
    X, C0 = _dup_data()
    labels, _, _ = K.assign(K.pack(X), X.shape[0], C0)
    C = C0.clone()
    counts, _ = K.update(X, labels, C)
    cnt = counts.cpu().numpy().tolist()
    assert sorted(i for i, x in enumerate(cnt) if x == 0) == [1, 3, 5, 8]
    before = C.cpu().numpy()
    seed, it = 987654321, 3
    ref_c, ref_n, hosts = _split_ref(before, cnt, seed, it)
    K.split(C, counts, seed, it)
    assert set(hosts) == {1, 3, 5, 8}
    got = C.cpu().numpy()
    assert np.array_equal(got.view(np.int32), ref_c.view(np.int32))
    assert counts.cpu().numpy().tolist() == ref_n
    for ci, cj in hosts.items():
        assert not np.array_equal(got[ci], got[cj])
    assert np.isfinite(got).all()
    # whole runs through empties: finite and the same bits twice
    r1 = K._kmeans(X, 10, niter=10, seed=5, init=C0)
    r2 = K._kmeans(X, 10, niter=10, seed=5, init=C0)
    assert torch.isfinite(r1["centres"]).all()
    assert torch.equal(r1["centres"].view(torch.int32), r2["centres"].view(torch.int32))
    assert torch.equal(r1["labels"], r2["labels"])
    assert np.array_equal(r1["objectives"], r2["objectives"])


# ---- whole runs against scikit-learn's Lloyd runs -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["d2", "d16", "d264"])
def test_whole_runs_match_sklearn(name):
    K = _K()
    g = _golden()
    X = torch.from_numpy(g[f"lloyd_{name}_X"]).to(DEV)
    init = torch.from_numpy(g[f"lloyd_{name}_init"]).to(DEV)
    niter = int(g[f"lloyd_{name}_niter"])
    res = K._kmeans(X, init.shape[0], niter=niter, seed=0, init=init)
    assert res["train_idx"] is None
    lab = res["labels"].cpu().numpy()
    assert np.array_equal(lab, g[f"lloyd_{name}_labels"])
    Xd, Cd = X.double(), res["centres"].double()
    inertia = float(((Xd - Cd[res["labels"]]) ** 2).sum())
    ref = float(g[f"lloyd_{name}_inertia"])
    assert abs(inertia - ref) <= 1e-5 * ref, (inertia, ref)


def test_objective_non_increasing_on_overlapping_data():
    K = _K()
    X = gmm(20000, 64, 0.5).to(DEV)
    res = K._kmeans(X, 200, niter=20, seed=3)
    o = res["objectives"][0]
    assert np.all(o[1:] <= o[:-1] * (1 + 1e-6)), o


# ---- training subsample, float64 input, ARI on the device path ----------------------------------------------------------

def test_training_subsample():
    K = _K()
    X = gmm(300_000, 16, 2.0).to(DEV)
    res = K._kmeans(X, 100, niter=3, seed=77)
    ref = np.sort(np.random.Generator(np.random.PCG64([77, 0])).choice(300_000, 25_600, replace=False))
    assert np.array_equal(res["train_idx"], ref)
    assert res["labels"].shape == (300_000,)
    assert int(res["labels"].min()) >= 0 and int(res["labels"].max()) < 100
    # the final labels cover every row: they are the nearest kept centre of each of the N rows
    lab_ref, _, _ = K.assign(K.pack(X), 300_000, res["centres"])
    assert torch.equal(res["labels"], lab_ref.long())
    small = K._kmeans(X[:20_000].contiguous(), 100, niter=3, seed=77)
    assert small["train_idx"] is None and small["labels"].shape == (20_000,)


def test_float64_input_equals_float32_cast():
    from torchdr_amd import kmeans_ari

    X = gmm(5000, 20, 1.0).double().to(DEV)
    y = (torch.arange(5000) % 50).to(DEV)
    s64, l64 = kmeans_ari(X, y, random_state=9)
    s32, l32 = kmeans_ari(X.float(), y, random_state=9)
    assert torch.equal(l64, l32) and torch.equal(s64, s32)


def test_ari_device_path_matches_fixture():
    K = _K()
    g = _golden()
    for i, ref in enumerate(g["ari_score"]):
        p = torch.from_numpy(g[f"ari_pred_{i}"]).to(DEV)
        t = torch.from_numpy(g[f"ari_true_{i}"]).to(DEV)
        got = K.ari_from_sums(*K.pair_sums(p, t))
        assert abs(got - ref) <= np.spacing(abs(ref)) + 1e-300, (i, got, ref)
    gg = np.random.default_rng(300_000)     # make_kmeans_golden.big_pair
    true = gg.integers(0, 10, 300_000)
    pred = true.copy()
    flip = gg.random(300_000) < 0.3
    pred[flip] = gg.integers(0, 10, int(flip.sum()))
    got = K.ari_from_sums(*K.pair_sums(torch.from_numpy(pred).to(DEV), torch.from_numpy(true).to(DEV)))
    ref = float(g["ari_big_score"])
    assert abs(got - ref) <= np.spacing(ref)


# ---- quality band and scale ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,scale", [("separated", 2.0), ("overlapping", 0.5)])
def test_quality_band(name, scale):
    from torchdr_amd import kmeans_ari

    X = gmm(20000, 64, scale).to(DEV)
    y = (torch.arange(20000) % 200).to(DEV)
    # one run's ARI spreads by ~0.05 with the seed on these mixtures: both sides are means over enough seeds (sklearn: 20,
    # recorded; here: 10) that the 0.02 band measures the algorithm, not the draw
    scores = [float(kmeans_ari(X, y, random_state=s)[0]) for s in range(10)]
    ref = float(_golden()[f"quality_{name}"].mean())
    assert np.mean(scores) >= ref - 0.02, (scores, ref)


def test_scale_1m():
    from torchdr_amd import kmeans_ari

    X = gmm(1_000_000, 128, 2.0).to(DEV)
    y = (torch.arange(1_000_000) % 1000).to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s1, l1 = kmeans_ari(X, y, random_state=0)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    s2, l2 = kmeans_ari(X, y, random_state=0)
    assert torch.isfinite(s1) and torch.equal(s1, s2) and torch.equal(l1, l2)
    assert wall < 120.0, wall    # a guard against a pathological slowdown, not a performance claim
