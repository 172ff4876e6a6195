"""K-means clustering + adjusted Rand index (reference ``eval/kmeans.py:22-173``), without faiss or torchmetrics.

The reference trains ``faiss.Kmeans`` on a host copy of X and scores it with torchmetrics' ``AdjustedRandScore``.  Here
faiss's documented procedure runs on ``csrc/tdr_kmeans.hip``:

1. Training set: all rows, or 256 * C distinct rows when N > 256 * C (faiss's ``max_points_per_centroid``).
2. Initial centres: C distinct training rows; run r of ``nredo`` has its own draw.
3. ``niter`` Lloyd iterations: assignment (squared L2, ties to the lower centre index), mean update, faiss's
   empty-cluster split.
4. A run's objective is the sum of squared distances of its last assignment; the run with the lowest one is kept.
5. Every row of X is assigned to the kept centres.

faiss's random streams cannot be reproduced without faiss; the draws are (seed = ``random_state`` or
``np.random.randint(2**31)``)::

    rows   = np.sort(Generator(PCG64([seed, 0])).choice(N, 256 * C, replace=False))      # only when N > 256 * C
    g      = Generator(PCG64([seed, 1 + r]))                                           # run r
    init   = g.choice(n_train, C, replace=False)        # centre i starts at training row init[i]
    split  = int(g.integers(0, 2**63))                  # seed of the run's empty-cluster draws (tdr_kmeans_split_f32)
"""

from typing import Optional, Union

import numpy as np
import torch

from torchdr_amd import _lib
from torchdr_amd.utils.wrappers import to_torch

MAX_POINTS_PER_CENTROID = 256
_BINCOUNT_MAX = 1 << 26   # contingency tables up to this many cells are a dense bincount, larger ones a sparse unique


def train_indices(seed: int, n: int, n_clusters: int):
    """Sorted training rows (int64) when N > 256 * C, else None (all rows)."""
    m = MAX_POINTS_PER_CENTROID * n_clusters
    if n <= m:
        return None
    g = np.random.Generator(np.random.PCG64([int(seed), 0]))
    return np.sort(g.choice(n, m, replace=False)).astype(np.int64)


def run_draws(seed: int, r: int, n_train: int, n_clusters: int):
    """(initial training rows of run r, seed of its empty-cluster draws)."""
    g = np.random.Generator(np.random.PCG64([int(seed), 1 + int(r)]))
    init = g.choice(n_train, n_clusters, replace=False).astype(np.int64)
    return init, int(g.integers(0, 2**63))


def _resolve_device(X, device):
    """CPU input goes to the current HIP device (as eval/silhouette.py); there is no CPU path."""
    if device is not None:
        device = torch.device(device)
        if device.type == "cpu":
            device = None
    if device is None:
        if isinstance(X, torch.Tensor) and X.is_cuda:
            device = X.device
        else:
            if not torch.cuda.is_available():
                raise RuntimeError(
                    "[torchdr_amd] kmeans: no HIP device is available; this build has no CPU path."
                )
            device = torch.device("cuda", torch.cuda.current_device())
    return device


def pack(X: torch.Tensor):
    """Tile images of the fp32 rows X (n, d): ``tdr_pack_rows_f32`` for d <= 256, ``tdr_pack_rows_wide_f32`` above."""
    L = _lib.lib()
    n, d = X.shape
    wide = d > 256
    nfl = L.tdr_packed_floats_wide(n, d) if wide else L.tdr_packed_floats(n, d)
    data = torch.empty(nfl, dtype=torch.float32, device=X.device)
    fn = L.tdr_pack_rows_wide_f32 if wide else L.tdr_pack_rows_f32
    _lib.check(fn(_lib.ptr(X), n, d, X.stride(0), _lib.ptr(data), None, _lib.stream_ptr()), fn.__name__)
    return data


def assign(xp, n: int, centres: torch.Tensor, obj: Optional[torch.Tensor] = None, cp=None):
    """Nearest centre of the n packed rows ``xp``: (labels int32, squared distances fp32, objective float64 (1,)).
    ``obj`` may be a float64 slot to write the objective into; ``cp`` the centres' packed images if already made."""
    L = _lib.lib()
    c, d = centres.shape
    dev = centres.device
    if cp is None:
        cp = pack(centres)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    if obj is None:
        obj = torch.empty(1, dtype=torch.float64, device=dev)
    ws_bytes = int(L.tdr_kmeans_assign_ws_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(L.tdr_kmeans_assign_f32(_lib.ptr(xp), n, _lib.ptr(cp), c, d, _lib.ptr(labels), _lib.ptr(dist), _lib.ptr(obj),
                                       _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), "tdr_kmeans_assign_f32")
    return labels, dist, obj


def update(X: torch.Tensor, labels: torch.Tensor, centres: torch.Tensor):
    """Mean of every non-empty cluster into ``centres`` (in place); returns (counts int32, perm int32)."""
    L = _lib.lib()
    n, d = X.shape
    c = centres.shape[0]
    counts = torch.empty(c, dtype=torch.int32, device=X.device)
    perm = torch.empty(n, dtype=torch.int32, device=X.device)
    ws_bytes = int(L.tdr_kmeans_update_ws_bytes(n, c, d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=X.device)
    _lib.check(L.tdr_kmeans_update_f32(_lib.ptr(X), n, d, X.stride(0), _lib.ptr(labels), c, _lib.ptr(centres), _lib.ptr(counts),
                                       _lib.ptr(perm), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), "tdr_kmeans_update_f32")
    return counts, perm


def split(centres: torch.Tensor, counts: torch.Tensor, seed: int, it: int):
    """faiss's empty-cluster split, in place (``tdr_kmeans_split_f32``)."""
    c, d = centres.shape
    _lib.check(_lib.lib().tdr_kmeans_split_f32(_lib.ptr(centres), c, d, _lib.ptr(counts), seed, it, _lib.stream_ptr()),
               "tdr_kmeans_split_f32")


def _kmeans(X: torch.Tensor, n_clusters: int, niter: int = 20, nredo: int = 1, seed: int = 0, verbose: bool = False,
            init: Optional[torch.Tensor] = None):
    """Lloyd k-means of the fp32 rows X (on a HIP device).  ``init`` (C, d) replaces every run's drawn initial centres.
    Returns a dict: labels (N, int64) of all rows, centres, train_idx (None = all rows), init_idx (per run), split_seed
    (per run), objectives (nredo, niter) float64 on the host, best (the kept run)."""
    X = X.contiguous()
    n, d = X.shape
    C = int(n_clusters)
    dev = X.device
    tidx = train_indices(seed, n, C)
    train = X if tidx is None else X[torch.as_tensor(tidx, device=dev)].contiguous()
    n_train = train.shape[0]
    xp = pack(train)
    objs = torch.zeros((nredo, max(niter, 1)), dtype=torch.float64, device=dev)
    runs, init_idx, split_seeds = [], [], []
    for r in range(nredo):
        rows, sseed = run_draws(seed, r, n_train, C)
        init_idx.append(rows)
        split_seeds.append(sseed)
        if init is not None:
            centres = init.to(device=dev, dtype=torch.float32).contiguous().clone()
        else:
            centres = train[torch.as_tensor(rows, device=dev)].contiguous()
        for it in range(niter):
            labels, _, _ = assign(xp, n_train, centres, obj=objs[r, it:it + 1])
            counts, _ = update(train, labels, centres)
            split(centres, counts, sseed, it)
            if verbose:
                print(f"[torchdr_amd] kmeans run {r} iteration {it}: objective {float(objs[r, it]):.6g}")
        if niter == 0:
            assign(xp, n_train, centres, obj=objs[r, 0:1])
        runs.append(centres)
    last = objs[:, -1].cpu().numpy()
    best = int(np.argmin(last))
    labels, _, _ = assign(pack(X) if tidx is not None else xp, n, runs[best])
    return dict(labels=labels.long(), centres=runs[best], train_idx=tidx, init_idx=init_idx, split_seed=split_seeds,
                objectives=objs.cpu().numpy()[:, :niter], best=best)


def pair_sums(pred: torch.Tensor, true: torch.Tensor):
    """(S, A, B, N) of the contingency table n_ij of (pred, true) as Python ints: S = sum n_ij^2, A = sum of squared
    row sums (pred), B = sum of squared column sums (true).  int64 sums on the device, one read to the host."""
    _, p = torch.unique(pred.reshape(-1), return_inverse=True)
    _, t = torch.unique(true.reshape(-1), return_inverse=True)
    n = p.numel()
    Lp = int(p.max()) + 1 if n else 0
    Lt = int(t.max()) + 1 if n else 0
    cell = p * Lt + t
    if Lp * Lt <= _BINCOUNT_MAX:
        nij = torch.bincount(cell, minlength=Lp * Lt)
    else:
        _, nij = torch.unique(cell, return_counts=True)
    a = torch.bincount(p, minlength=Lp)
    b = torch.bincount(t, minlength=Lt)
    sums = torch.stack([(nij * nij).sum(), (a * a).sum(), (b * b).sum()]).cpu().tolist()
    return int(sums[0]), int(sums[1]), int(sums[2]), int(n)


def ari_from_sums(S: int, A: int, B: int, N: int) -> float:
    """sklearn's pair-confusion ARI in exact integers, divided once in float64 (torchmetrics' int64 products overflow
    from N ~ 1e5)."""
    tp = S - N
    fp = A - S
    fn = B - S
    tn = N * N - fp - fn - S
    if fn == 0 and fp == 0:
        return 1.0
    return 2 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def kmeans_ari(
    X: Union[torch.Tensor, np.ndarray],
    labels: Union[torch.Tensor, np.ndarray],
    n_clusters: Optional[int] = None,
    niter: int = 20,
    nredo: int = 1,
    device: Optional[str] = None,
    random_state: Optional[int] = None,
    verbose: bool = False,
):
    """K-means of X (float32 working precision) and the adjusted Rand index of its clusters against ``labels``
    (reference ``eval/kmeans.py:22-173``).

    Returns (score, predicted labels): a Python float and an int64 ``np.ndarray`` if either input is not a tensor, else a
    0-d float32 tensor and an int64 tensor, both on ``device`` (default: X's device).  Raises ``ValueError`` if
    ``n_clusters`` is below 1 or above the number of samples."""
    input_is_numpy = not isinstance(X, torch.Tensor) or not isinstance(labels, torch.Tensor)
    X = to_torch(X)
    labels = to_torch(labels).squeeze()
    out_device = torch.device(device) if device is not None else X.device
    n_samples = X.shape[0]
    if n_clusters is None:
        n_clusters = int(torch.unique(labels).numel())
    if n_clusters < 1:
        raise ValueError(f"n_clusters must be at least 1, got {n_clusters}")
    if n_clusters > n_samples:
        raise ValueError(f"n_clusters ({n_clusters}) cannot be greater than n_samples ({n_samples})")
    if random_state is not None:
        np.random.seed(random_state)
    seed = random_state if random_state is not None else np.random.randint(2**31)

    dev = _resolve_device(X, device)
    with torch.no_grad():
        Xf = X.detach().reshape(n_samples, -1).to(device=dev, dtype=torch.float32)
        res = _kmeans(Xf, n_clusters, niter=niter, nredo=nredo, seed=int(seed), verbose=verbose)
        pred = res["labels"]
        true = labels.detach().reshape(-1).long().to(dev)
        score = ari_from_sums(*pair_sums(pred, true))
    if input_is_numpy:
        return float(score), pred.cpu().numpy()
    return torch.tensor(score, dtype=torch.float32, device=out_device), pred.to(out_device)
