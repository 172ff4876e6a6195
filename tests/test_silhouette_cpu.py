"""silhouette_samples / silhouette_score without a GPU: signatures, host-side argument checks, the C ABI's argument
checks, the missing-GPU failure, and the host-side path choice and segment-fold rule."""

import ctypes
import inspect
import json
import os
import random

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _sig(obj):
    ps = inspect.signature(obj).parameters
    return [[k, None if v.default is inspect._empty else repr(v.default)] for k, v in ps.items()]


def test_signatures_match_reference():
    import torchdr_amd
    from torchdr_amd import eval as E

    with open(os.path.join(HERE, "golden", "silhouette_signatures.json")) as f:
        ref = json.load(f)
    assert _sig(E.silhouette_samples) == ref["eval.silhouette_samples"]
    assert _sig(E.silhouette_score) == ref["eval.silhouette_score"]
    assert torchdr_amd.silhouette_samples is E.silhouette_samples
    assert torchdr_amd.silhouette_score is E.silhouette_score
    assert E.admissible_LIST_METRICS == ["euclidean", "manhattan", "hyperbolic", "precomputed"]


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt at device work fails loudly here, so the errors below are shown to come first."""
    from torchdr_amd.eval import silhouette as S

    def boom(*a, **k):
        raise AssertionError("device work started before the argument check")

    monkeypatch.setattr(S, "_silhouette", boom)
    return S


def test_argument_errors_before_device_work(no_device):
    S = no_device
    X = np.random.default_rng(0).normal(size=(12, 3))
    y = np.arange(12) % 3
    with pytest.raises(ValueError, match="must be in"):
        S.silhouette_samples(X, y, metric="whatever")
    with pytest.raises(ValueError, match="must be in"):
        S.silhouette_score(X, y, metric="cosine")
    with pytest.raises(ValueError, match="'hyperbolic' distance is not supported"):
        S.silhouette_samples(X, y, metric="hyperbolic")
    with pytest.raises(ValueError, match="square matrix"):
        S.silhouette_samples(X, y, metric="precomputed")
    with pytest.raises(ValueError, match="square matrix"):
        S.silhouette_score(X, y, metric="precomputed", sample_size=5)
    with pytest.raises(ValueError):
        S.silhouette_score(X, y, sample_size=13)   # larger than the population, as random.sample


def test_keops_precomputed_warns(no_device):
    S = no_device
    D = np.zeros((6, 6))
    with pytest.warns(UserWarning, match="backend 'keops' not supported"):
        with pytest.raises(AssertionError):
            S.silhouette_samples(D, np.arange(6) % 2, metric="precomputed", backend="keops")


def test_sample_subset_is_the_reference_draw(monkeypatch):
    """sample_size draws random.seed(rs); random.sample(range(n), k) -- without touching the global state."""
    from torchdr_amd.eval import silhouette as S

    seen = {}

    def fake(X, labels, weights, metric, device, warn, **kw):
        seen["X"], seen["labels"] = X, labels
        return torch.zeros(X.shape[0], dtype=torch.float64)

    monkeypatch.setattr(S, "_silhouette", fake)
    monkeypatch.setattr(S, "_mean", lambda s: s.mean())
    X = np.arange(40, dtype=np.float64).reshape(20, 2)
    y = np.arange(20) % 4
    state = random.getstate()
    S.silhouette_score(X, y, sample_size=7, random_state=5)
    assert random.getstate() == state
    random.seed(5)
    want = random.sample(range(20), 7)
    assert seen["X"][:, 0].numpy().tolist() == [2.0 * i for i in want]
    assert seen["labels"].numpy().tolist() == [i % 4 for i in want]


def test_no_gpu_fails_loudly(monkeypatch):
    from torchdr_amd.eval import silhouette as S

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.silhouette_samples(np.zeros((4, 2)), np.array([0, 0, 1, 1]))


def test_abi_argument_checks():
    from torchdr_amd import _lib

    L = _lib.lib()
    p, null = ctypes.c_void_p(64), ctypes.c_void_p(0)
    big = 1 << 40
    assert L.tdr_silhouette_workspace_bytes(1000, 3, 4) == 3 * 1000 * (4 * 4 + 8)
    assert L.tdr_silhouette_workspace_bytes(1000, 3, 8) == 3 * 1000 * (4 * 8 + 8)
    assert L.tdr_silhouette_workspace_bytes(1000, 3, 2) == 0
    ws = L.tdr_silhouette_workspace_bytes(1000, 1, 4)
    assert L.tdr_silhouette_direct_f32(null, 1000, 2, p, null, p, 0, 1, p, ws, null) == -1       # no points
    assert L.tdr_silhouette_direct_f32(p, 1000, 2, p, null, p, 2, 1, p, ws, null) == -1          # unknown metric
    assert L.tdr_silhouette_direct_f32(p, 1000, 5, p, null, p, 0, 1, p, ws, null) == -2          # unpadded width
    assert L.tdr_silhouette_direct_f64(p, 1000, 2, p, null, p, 0, 7, p, big, null) == -1         # 7 segments of 1000 columns do not exist
    assert L.tdr_silhouette_direct_f64(p, 0, 2, p, null, p, 0, 1, p, ws, null) == -1
    assert L.tdr_silhouette_direct_f32(p, 1 << 32, 2, p, null, p, 0, 1, p, big, null) == -2      # beyond int32 ids
    assert L.tdr_silhouette_precomputed_f32(p, 10, 20, p, p, null, p, p, big, null) == -1        # row stride < n
    assert L.tdr_silhouette_precomputed_f64(p, 20, 20, null, p, null, p, p, big, null) == -1
    assert L.tdr_silhouette_finish_f32(p, big, 20, 0, p, null, p, p, p, p, null, null, null) == -1
    assert L.tdr_silhouette_finish_f64(p, big, 20, 1, p, null, p, p, p, null, null, null, null) == -1
    assert L.tdr_silhouette_label_weights_f32(null, null, 4, p, null) == -1
    assert L.tdr_silhouette_label_weights_f64(null, p, 0, p, null) == -1
    assert L.tdr_silhouette_mean_f32(p, 0, p, null) == -1
    assert L.tdr_silhouette_mean_f64(null, 5, p, null) == -1


def test_path_choice():
    from torchdr_amd.eval import silhouette as S

    for d in (1, 2, 3, 16, 128, 300, 1000):
        for dt in (torch.float32, torch.float64):
            for m in ("euclidean", "manhattan"):
                assert S._choose_path(d, dt, m) == "direct"
            assert S._choose_path(d, dt, "precomputed") == "precomputed"
    assert [S._padded_dim(d) for d in (1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 300)] == [2, 2, 3, 4, 8, 8, 16, 16, 32, 64, 304]


def test_segment_count_rule():
    """Segments are whole 64-column tiles, none empty, and the count matches the kernel's own cut (ceil(ceil(n / want) / 64)
    * 64 columns per segment)."""
    from torchdr_amd.eval import silhouette as S

    for n in (1, 63, 64, 65, 1000, 4097, 20_000, 200_000, 1_000_000):
        for want in (None, 1, 2, 3, 7, 64, 10_000):
            k = S._n_segments(n, want)
            assert k >= 1
            seg = -(-(-(-n // max(1, min(want or k, n)))) // 64) * 64 if want else None
            if want is not None:
                assert k == -(-n // seg)
            cols = -(-(-(-n // k)) // 64) * 64
            assert -(-n // cols) == k and (k - 1) * cols < n
    assert S._n_segments(1_000_000) <= 2      # 3907 row blocks nearly fill the chip on their own
    assert S._n_segments(20_000) > 1


def _brute(dw, lab, own, W):
    runs = {}
    for x, l in zip(dw, lab):
        runs[l] = runs.get(l, 0.0) + x
    b = min((s / W[l] for l, s in runs.items() if l != own), default=float("inf"))
    return runs.get(own, 0.0), b


@pytest.mark.parametrize("seed", range(6))
def test_segment_fold_rule(seed):
    """Cutting the sorted columns at arbitrary places and folding the segment states in order gives the unsegmented
    sums: runs that span several segments, segments inside one run, singletons, a single label."""
    from torchdr_amd.eval import silhouette as S

    g = np.random.default_rng(seed)
    n = int(g.integers(1, 60))
    L = int(g.integers(1, 8)) if seed != 5 else n
    lab = np.sort(g.integers(0, L, size=n)) if seed != 5 else np.arange(n)
    dw = g.random(n)
    W = {int(l): float(g.random() + 0.5) for l in np.unique(lab)}
    for own in np.unique(lab):
        own = int(own)
        want_own, want_b = _brute(dw, lab.tolist(), own, W)
        for n_cuts in range(0, min(n, 6)):
            cuts = sorted(set(g.integers(1, n, size=n_cuts).tolist())) if n > 1 else []
            bounds = [0] + cuts + [n]
            states = [S._segment_state(dw[a:b].tolist(), lab[a:b].tolist(), own) for a, b in zip(bounds[:-1], bounds[1:])]
            got_own, got_b = S._fold_segments(states, own, W)
            assert got_own == pytest.approx(want_own, rel=1e-12, abs=1e-12)
            assert got_b == pytest.approx(want_b, rel=1e-12)
