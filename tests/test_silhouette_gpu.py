"""Exact silhouette on the GPU: parity with the reference's values (tests/golden/silhouette.npz), and a float64 restatement
of the definition computed in chunks, across dimensions, label counts, paths, segment splits, dtypes and weights."""

import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests.conftest import gmm, regime_data

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "silhouette.npz"))
    return {k: z[k] for k in z.files}


def _restate(X, inv, w, rows, metric):
    """float64 a, b, s of the rows `rows` against all points (the documented definition; d_ii = 0)."""
    X = X.to(torch.float64)
    n = X.shape[0]
    L = int(inv.max()) + 1
    w = torch.ones(n, dtype=torch.float64, device=X.device) if w is None else w.to(torch.float64)
    W = torch.zeros(L, dtype=torch.float64, device=X.device).index_add_(0, inv, w)
    cnt = torch.bincount(inv, minlength=L)
    A, B = [], []
    chunk = max(16, min(1024, (1 << 27) // max(n, L)))
    if metric == "manhattan":   # formed by broadcasting, not torch.cdist(p=1): (chunk, n, d) in float64, <= 2 GiB
        chunk = max(1, min(chunk, (1 << 28) // (n * X.shape[1])))
    for r in rows.split(chunk):
        if metric == "precomputed":
            D = X[r].clone()
        elif metric == "manhattan":
            D = (X[r][:, None, :] - X[None, :, :]).abs().sum(-1)
        else:
            D = torch.cdist(X[r], X)
            D[torch.arange(r.numel(), device=X.device), r] = 0.0
        S = torch.zeros(r.numel(), L, dtype=torch.float64, device=X.device).index_add_(1, inv, D * w)
        own = inv[r]
        so = S.gather(1, own[:, None])[:, 0]
        A.append(torch.where(cnt[own] > 1, so / (W[own] - w[r]), torch.zeros_like(so)))
        Sb = S / W
        Sb.scatter_(1, own[:, None], float("inf"))
        B.append(Sb.min(1).values)
    a, b = torch.cat(A), torch.cat(B)
    return a, b, torch.nan_to_num((b - a) / torch.maximum(a, b), 0.0)


def _check(X, labels, w=None, metric="euclidean", rows=None, **kw):
    from torchdr_amd.eval.silhouette import _silhouette

    s, a, b = _silhouette(X, labels, w, metric, None, False, _return_ab=True, **kw)
    _, inv = torch.unique(labels.to(X.device), return_inverse=True)
    n = X.shape[0]
    rows = torch.arange(n, device=X.device) if rows is None else rows
    a64, b64, s64 = _restate(X, inv, w, rows, metric)
    tol = 1e-10 if X.dtype == torch.float64 else 1e-5
    assert s.dtype == X.dtype and s.device == X.device
    np.testing.assert_allclose(a[rows].double().cpu(), a64.cpu(), rtol=tol, atol=1e-300)
    np.testing.assert_allclose(b[rows].double().cpu(), b64.cpu(), rtol=tol, atol=1e-300)
    assert float((s[rows].double() - s64).abs().max()) <= tol
    return s


# ---- parity with the reference -----------------------------------------------------------------------------------------

def _case(golden, name):
    xk, lk, wk, metric, ss, rs = json.loads(str(golden["cases"]))[name]
    return golden[xk], golden[lk], (None if wk is None else golden[wk]), metric, ss, rs


@pytest.mark.parametrize("name", ["eu_int", "l1_int", "eu_float", "eu_one", "eu_sample", "l1_sample", "pre_int", "pre_sample",
                                  "id_eu", "id_l1", "id_pre", "id2_eu", "id2_eu_w", "id2_l1", "id2_pre"])
def test_reference_parity(golden, name):
    from torchdr_amd import silhouette_samples, silhouette_score

    X, lab, w, metric, ss, rs = _case(golden, name)
    # the reference's euclidean form leaves a self-distance d_ii of up to `selfdist` (recorded with it; ~1e-7 in float64),
    # which enters its a_i; the HIP path has d_ii = 0 exactly, so that much is allowed on top of the budget
    slack = float(golden.get(f"{name}_selfdist64", 0.0))
    for dt, tol in ((np.float64, 1e-10 + slack), (np.float32, 1e-5 + slack)):
        Xd = X.astype(dt)
        wd = None if w is None else w.astype(dt)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if ss is None:
                s = silhouette_samples(torch.from_numpy(Xd).to(DEV), torch.from_numpy(lab).to(DEV),
                                       None if wd is None else torch.from_numpy(wd).to(DEV), metric, None, None, False)
                assert s.dtype == torch.from_numpy(Xd).dtype and s.is_cuda
                np.testing.assert_allclose(s.double().cpu().numpy(), golden[f"{name}_s64"], rtol=0, atol=tol)
            score = silhouette_score(Xd, lab, wd, metric, None, None, ss, rs, False)
        assert isinstance(score, float)
        assert abs(score - float(golden[f"{name}_score64"])) <= tol


def test_return_types_and_devices(golden):
    from torchdr_amd import silhouette_samples, silhouette_score

    X, lab = golden["X"], golden["lab_int"]
    s = silhouette_samples(X, lab, warn=False)                  # numpy in: a tensor on the current HIP device, X's dtype
    assert isinstance(s, torch.Tensor) and s.is_cuda and s.dtype == torch.float64 and not s.requires_grad
    s32 = silhouette_samples(X.astype(np.float32), lab, warn=False, device=DEV)
    assert s32.dtype == torch.float32 and s32.is_cuda
    Xt = torch.from_numpy(X).to(DEV).requires_grad_(True)
    st = silhouette_score(Xt, torch.from_numpy(lab).to(DEV), warn=False)
    assert isinstance(st, torch.Tensor) and st.dim() == 0 and st.dtype == torch.float64 and not st.requires_grad
    assert isinstance(silhouette_score(X, lab, warn=False), float)
    sc = silhouette_score(torch.from_numpy(X), torch.from_numpy(lab), warn=False)   # a CPU tensor runs on the HIP device
    assert isinstance(sc, torch.Tensor) and sc.is_cuda
    from torchdr_amd.distance import FaissConfig

    scores = [silhouette_score(X, lab, backend=b, warn=False) for b in (None, "keops", "faiss", FaissConfig())]
    assert len(set(scores)) == 1 and abs(scores[0] - float(golden["eu_int_score64"])) <= 1e-10 + float(golden["eu_int_selfdist64"])


def test_warnings(golden):
    from torchdr_amd import silhouette_samples

    X, lab = golden["X"], golden["lab_int"]
    with pytest.warns(UserWarning, match="ill-defined intra-cluster mean distance"):
        silhouette_samples(X, lab)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        silhouette_samples(X, lab, warn=False)
        silhouette_samples(golden["X"], golden["lab_one"])    # no singleton, no warning


def test_sample_subset(golden):
    """sample_size evaluates exactly the reference's subset (the score of the subset computed directly)."""
    import random

    from torchdr_amd import silhouette_samples, silhouette_score

    X, lab = golden["X"], golden["lab_int"]
    idx = random.Random(7).sample(range(X.shape[0]), 100)
    direct = silhouette_samples(X[idx], lab[idx], warn=False).double().mean().item()
    assert abs(silhouette_score(X, lab, sample_size=100, random_state=7, warn=False) - direct) <= 1e-12


# ---- against the float64 restatement -------------------------------------------------------------------------------------

SHAPES = [(20_000, 2, 10), (20_000, 3, 1000), (20_000, 16, 2), (20_000, 64, 10_000), (20_000, 128, 10), (20_000, 300, 1000),
          (200_000, 2, 10), (200_000, 3, 100_000)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("metric", ["euclidean", "manhattan"])
@pytest.mark.parametrize("n,d,L", SHAPES)
def test_restatement_shapes(n, d, L, metric, dtype):
    g = torch.Generator().manual_seed(n + d + L)
    labels = torch.randint(0, L, (n,), generator=g)
    centers = torch.randn(L, d, generator=g) * 2.0
    X = (centers[labels] + 0.5 * torch.randn(n, d, generator=g)).to(DEV, dtype)
    rows = None if n <= 20_000 else torch.randperm(n, generator=g)[:2048].to(DEV)
    _check(X, labels.to(DEV), None, metric, rows)


@pytest.mark.parametrize("name", ["gmm2", "overlap", "swiss", "heavytail"])
def test_regime_data(name):
    X, lab = regime_data(name, 20_000)
    for dtype in (torch.float32, torch.float64):
        _check(X.to(DEV, dtype), lab.to(DEV))


@pytest.mark.parametrize("n_seg", [1, 2, 7, 64])
def test_forced_segments(n_seg):
    X = gmm(20_000, 8, 2.0, seed=3).to(DEV)
    lab = (torch.arange(20_000) % 200).to(DEV)
    s = _check(X, lab, _n_seg=n_seg)
    s_auto = _check(X, lab)
    assert float((s - s_auto).abs().max()) <= 2e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_forced_paths(dtype):
    """The direct path and the precomputed path (on the distance matrix of the same points) agree with the restatement."""
    X = gmm(4000, 12, 1.0, seed=5).to(DEV, dtype)
    lab = (torch.arange(4000) % 37).to(DEV)
    s_direct = _check(X, lab, _path="direct")
    D = torch.cdist(X.double(), X.double(), compute_mode="donot_use_mm_for_euclid_dist").to(dtype)
    D.fill_diagonal_(0.0)
    s_pre = _check(D, lab, metric="precomputed", _path="precomputed")
    tol = 1e-10 if dtype == torch.float64 else 2e-5
    assert float((s_direct - s_pre).abs().max()) <= tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_weights(dtype):
    g = torch.Generator().manual_seed(9)
    n = 20_000
    X = gmm(n, 5, 1.0, seed=9).to(DEV, dtype)
    lab = torch.randint(-5, 40, (n,), generator=g).to(DEV)
    w = (0.1 + 1.9 * torch.rand(n, generator=g)).to(DEV, dtype)
    _check(X, lab, w)
    _check(X, lab, w, metric="manhattan")
    from torchdr_amd import silhouette_samples

    uni = silhouette_samples(X, lab, torch.full((n,), 0.37, dtype=dtype, device=DEV), warn=False)
    plain = silhouette_samples(X, lab, warn=False)
    tol = 1e-12 if dtype == torch.float64 else 2e-6
    assert float((uni - plain).abs().max()) <= tol
    D = torch.cdist(X[:3000].double(), X[:3000].double(), compute_mode="donot_use_mm_for_euclid_dist").to(dtype)
    D.fill_diagonal_(0.0)
    _check(D, lab[:3000], w[:3000], metric="precomputed")


def test_determinism_and_permutation():
    from torchdr_amd.eval.silhouette import _silhouette

    for dtype, tol in ((torch.float32, 1e-5), (torch.float64, 1e-10)):
        X = gmm(30_000, 10, 1.0, seed=13).to(DEV, dtype)
        lab = (torch.arange(30_000) * 7919 % 300).to(DEV)
        s1 = _silhouette(X, lab, None, "euclidean", None, False, _n_seg=9)
        s2 = _silhouette(X, lab, None, "euclidean", None, False, _n_seg=9)
        assert torch.equal(s1, s2)
        p = torch.randperm(30_000, generator=torch.Generator().manual_seed(1)).to(DEV)
        sp = _silhouette(X[p], lab[p], None, "euclidean", None, False)
        assert float((sp - s1[p]).abs().max()) <= tol


def test_headline_one_million_points():
    """N = 1M, D = 2, 10 labels (a UMAP-like embedding): 512 sampled rows against an exact float64 row evaluation."""
    from torchdr_amd import silhouette_score

    n = 1_000_000
    g = torch.Generator().manual_seed(2026)
    lab = torch.randint(0, 10, (n,), generator=g)
    ang = lab.double() * (2 * np.pi / 10)
    X = torch.stack([6 * torch.cos(ang), 6 * torch.sin(ang)], 1) + torch.randn(n, 2, generator=g, dtype=torch.float64)
    X = X.float().to(DEV)
    rows = torch.randperm(n, generator=g)[:512].to(DEV)
    s = _check(X, lab.to(DEV), rows=rows)
    score = silhouette_score(X, lab.to(DEV), warn=False)
    assert abs(float(score) - s.double().mean().item()) <= 1e-6
