"""Silhouette coefficients and score (reference ``eval/silhouette.py:21-246``), exact and matrix-free on HIP.

The reference builds every ``n_i x n_j`` block of distances for each pair of labels.  Here the points are sorted by label
once, and ``csrc/tdr_silhouette.hip`` streams all N^2 pairs tile by tile, reducing each row on the fly: memory is
O(N D + N + L).  Same signatures, errors, warnings and return types as the reference, with one deliberate deviation on
weighted input: the documented definition

    a_i = sum_{j in C(i)} w_j d_ij / (W_C(i) - w_i),    b_i = min_{l != C(i)} sum_{j in l} w_j d_ij / W_l,

which equals the reference wherever the reference is well defined (uniform weights).
"""

import random
import warnings
from typing import Optional, Union

import numpy as np
import torch

from torchdr_amd import _lib
from torchdr_amd.utils.wrappers import to_torch

admissible_LIST_METRICS = ["euclidean", "manhattan", "hyperbolic", "precomputed"]

_METRIC_ID = {"euclidean": 0, "manhattan": 1}
_SMALL_DIMS = (2, 3, 4, 8, 16)
_SEG_TILE = 64           # columns of a scan segment are whole 64-column tiles
_TARGET_WORKGROUPS = 4096
_MIN_SEG_COLS = 1024


def _check_args(X, metric, backend, warn):
    """Host-side argument checks of the reference (:80-92, :1-2 of its distance dispatch), before any device work."""
    if metric not in admissible_LIST_METRICS:
        raise ValueError(f"metric = {metric} must be in {admissible_LIST_METRICS}")
    if metric == "hyperbolic":
        # the reference admits the name but its distance dispatch rejects it
        raise ValueError("[TorchDR] ERROR : The 'hyperbolic' distance is not supported.")
    if metric == "precomputed":
        if X.shape[0] != X.shape[1]:
            raise ValueError("X must be a square matrix with metric = 'precomputed'")
        if backend == "keops" and warn:
            warnings.warn(
                "[TorchDR] WARNING : backend 'keops' not supported with metric = 'precomputed'.",
                stacklevel=3,
            )


def _choose_path(d, dtype, metric):
    """Which kernel computes the distances: ``precomputed`` reads the given matrix, ``direct`` forms every distance from
    coordinate differences on the vector ALUs (any D, float32 and float64, euclidean and manhattan)."""
    if metric == "precomputed":
        return "precomputed"
    if metric in _METRIC_ID and dtype in (torch.float32, torch.float64):
        return "direct"
    raise ValueError(f"no silhouette path for metric={metric!r}, dtype={dtype}")


def _padded_dim(d):
    """Width of the transposed, zero-padded copy the direct kernels read (zero columns change no distance)."""
    for p in _SMALL_DIMS:
        if d <= p:
            return p
    return (d + 15) // 16 * 16


def _n_segments(n, want=None):
    """Number of column segments of a direct scan: enough workgroups to fill the chip (rows are taken 256 per workgroup),
    segments of at least _MIN_SEG_COLS columns.  The kernel cuts the columns into segments of
    ceil(ceil(n / want) / 64) * 64 columns; the count returned is the number of such segments (none empty)."""
    if want is None:
        blocks = (n + 255) // 256
        want = min(-(-_TARGET_WORKGROUPS // blocks), max(1, n // _MIN_SEG_COLS), 256)
    want = max(1, min(int(want), n))
    seg_cols = -(-(-(-n // want)) // _SEG_TILE) * _SEG_TILE
    return -(-n // seg_cols)


def _segment_state(dist_w, lab, own):
    """Partial state a scan leaves for one segment of sorted columns (restatement of SilScan in tdr_silhouette.hip, float64):
    (first label, first partial sum; min over the runs seen whole of sum / W; last label, last partial sum; own-label sum).
    `dist_w`: w_j d_ij over the segment, `lab`: its label ids (sorted).  The min needs W, so it is returned as the list
    of the whole runs (label, sum) and turned into a minimum by `_fold_segments`."""
    runs = []
    for x, l in zip(dist_w, lab):
        if runs and runs[-1][0] == l:
            runs[-1][1] += x
        else:
            runs.append([l, x])
    if len(runs) == 1:
        return (runs[0][0], runs[0][1], runs[1:-1], runs[0][0], 0.0)
    return (runs[0][0], runs[0][1], runs[1:-1], runs[-1][0], runs[-1][1])


def _fold_segments(states, own, W):
    """Fold segment states in order (restatement of sil_fold_state): returns (sum over the own label, b)."""
    open_lab, open_sum, minb, own_sum = None, 0.0, float("inf"), 0.0

    def close(lab, s):
        nonlocal minb, own_sum
        if lab is None:
            return
        if lab == own:
            own_sum += s
        else:
            minb = min(minb, s / W[lab])

    for lf, sf, middle, ll, sl in states:
        if lf == open_lab:
            open_sum += sf
        else:
            close(open_lab, open_sum)
            open_lab, open_sum = lf, sf
        for lab, s in middle:
            close(lab, s)
        if lf != ll:
            close(open_lab, open_sum)
            open_lab, open_sum = ll, sl
    close(open_lab, open_sum)
    return own_sum, minb


def _resolve_device(X, device):
    """CPU input goes to the current HIP device (as eval/neighborhood_preservation.py); there is no CPU path."""
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
                    "[torchdr_amd] silhouette: no HIP device is available; this build has no CPU path."
                )
            device = torch.device("cuda", torch.cuda.current_device())
    return device


def _silhouette(X, labels, weights=None, metric="euclidean", device=None, warn=True, _path=None, _n_seg=None,
                _return_ab=False):
    """Silhouette coefficients in X's dtype on the resolved device (original order).  `_path` ("direct" / "precomputed")
    and `_n_seg` (column segments of the direct scan) force the kernel choice for tests; `_return_ab` also returns a, b."""
    X = to_torch(X)
    out_dtype = X.dtype
    dev = _resolve_device(X, device)
    dtype = X.dtype if X.dtype in (torch.float32, torch.float64) else torch.float32
    with torch.no_grad():
        X = X.detach().to(device=dev, dtype=dtype)
        lab = torch.as_tensor(labels).squeeze().reshape(-1).to(dev)
        n = X.shape[0]
        if lab.numel() != n:
            raise ValueError(f"labels has {lab.numel()} entries for {n} samples")
        w = None
        if weights is not None:
            w = to_torch(weights).detach().squeeze().reshape(-1).to(device=dev, dtype=dtype)
            if w.numel() != n:
                raise ValueError(f"weights has {w.numel()} entries for {n} samples")

        uniq, inv = torch.unique(lab, return_inverse=True)
        L = uniq.numel()
        perm = torch.argsort(inv, stable=True)
        lab_s = inv[perm].to(torch.int32).contiguous()
        counts = torch.bincount(inv, minlength=L)
        starts = torch.zeros(L + 1, dtype=torch.int64, device=dev)
        starts[1:] = torch.cumsum(counts, 0)
        if warn and bool((counts == 1).any()):
            warnings.warn(
                "[TorchDR] WARNING : ill-defined intra-cluster mean distance as one cluster contains only one sample.",
                stacklevel=3,
            )
        w_s = w[perm].contiguous() if w is not None else None
        W = torch.empty(L, dtype=dtype, device=dev)
        sfx = "_f64" if dtype == torch.float64 else "_f32"
        L_ = _lib.lib()
        st = _lib.stream_ptr()
        _lib.check(getattr(L_, "tdr_silhouette_label_weights" + sfx)(_lib.ptr(w_s), _lib.ptr(starts), L, _lib.ptr(W), st),
                   "tdr_silhouette_label_weights")

        path = _path or _choose_path(X.shape[1] if X.dim() == 2 else 1, dtype, metric)
        if path == "precomputed":
            if metric != "precomputed":
                raise ValueError("the precomputed path needs metric='precomputed'")
            Dm = X if X.stride(1) == 1 else X.contiguous()
            n_seg = 1
            ws_bytes = L_.tdr_silhouette_workspace_bytes(n, n_seg, X.element_size())
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(getattr(L_, "tdr_silhouette_precomputed" + sfx)(
                _lib.ptr(Dm), Dm.stride(0), n, _lib.ptr(perm), _lib.ptr(lab_s), _lib.ptr(w_s), _lib.ptr(W),
                _lib.ptr(ws), ws_bytes, st), "tdr_silhouette_precomputed")
        elif path == "direct":
            if metric not in _METRIC_ID:
                raise ValueError(f"the direct path does not compute metric={metric!r}")
            Xf = X.reshape(n, -1)
            d = Xf.shape[1]
            dp = _padded_dim(d)
            XT = torch.zeros(dp, n, dtype=dtype, device=dev)
            XT[:d] = Xf[perm].t()
            n_seg = _n_segments(n, _n_seg)
            ws_bytes = L_.tdr_silhouette_workspace_bytes(n, n_seg, X.element_size())
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(getattr(L_, "tdr_silhouette_direct" + sfx)(
                _lib.ptr(XT), n, dp, _lib.ptr(lab_s), _lib.ptr(w_s), _lib.ptr(W), _METRIC_ID[metric], n_seg,
                _lib.ptr(ws), ws_bytes, st), "tdr_silhouette_direct")
        else:
            raise ValueError(f"unknown silhouette path {path!r}")

        s = torch.empty(n, dtype=dtype, device=dev)
        a = torch.empty(n, dtype=dtype, device=dev) if _return_ab else None
        b = torch.empty(n, dtype=dtype, device=dev) if _return_ab else None
        _lib.check(getattr(L_, "tdr_silhouette_finish" + sfx)(
            _lib.ptr(ws), ws_bytes, n, n_seg, _lib.ptr(lab_s), _lib.ptr(w_s), _lib.ptr(W), _lib.ptr(starts), _lib.ptr(perm),
            _lib.ptr(s), _lib.ptr(a), _lib.ptr(b), st), "tdr_silhouette_finish")
    s = s.to(out_dtype)
    if _return_ab:
        return s, a, b
    return s


def _mean(s):
    """Mean of the coefficients in float64, in a fixed reduction order, returned in their dtype."""
    out = torch.empty((), dtype=torch.float64, device=s.device)
    sc = s if s.dtype in (torch.float32, torch.float64) else s.float()
    fn = _lib.fn("tdr_silhouette_mean", sc.dtype)
    _lib.check(fn(_lib.ptr(sc.contiguous()), sc.numel(), _lib.ptr(out), _lib.stream_ptr()), "tdr_silhouette_mean")
    return out.to(s.dtype)


def silhouette_samples(
    X: Union[torch.Tensor, np.ndarray],
    labels: Union[torch.Tensor, np.ndarray],
    weights: Optional[Union[torch.Tensor, np.ndarray]] = None,
    metric: str = "euclidean",
    device: Optional[str] = None,
    backend=None,
    warn: bool = True,
):
    """Silhouette coefficient (b - a) / max(a, b) of every sample (reference ``eval/silhouette.py:21-163``).

    Every ``backend`` value runs the same exact HIP computation.  Returns a tensor in X's dtype, on ``device`` if given,
    else on X's device (CPU input: the current HIP device)."""
    _check_args(X, metric, backend, warn)
    return _silhouette(X, labels, weights, metric, device, warn)


def silhouette_score(
    X: Union[torch.Tensor, np.ndarray],
    labels: Union[torch.Tensor, np.ndarray],
    weights: Optional[Union[torch.Tensor, np.ndarray]] = None,
    metric: str = "euclidean",
    device: Optional[str] = None,
    backend=None,
    sample_size: Optional[int] = None,
    random_state: Optional[int] = None,
    warn: bool = True,
):
    """Mean silhouette coefficient (reference ``eval/silhouette.py:166-246``): a Python float for numpy X, else a 0-d
    tensor.  ``sample_size`` draws the reference's subset, ``random.Random(random_state).sample(range(n), sample_size)``,
    without touching the global random state."""
    input_is_numpy = not isinstance(X, torch.Tensor)
    _check_args(X, metric, backend, warn)
    if sample_size is None:
        coefficients = _silhouette(X, labels, weights, metric, device, warn)
    else:
        indices = random.Random(random_state).sample(range(X.shape[0]), sample_size)
        idx = np.asarray(indices, dtype=np.int64)
        X_t = to_torch(X)
        it = torch.as_tensor(idx, device=X_t.device)
        sub_X = X_t[it][:, it] if metric == "precomputed" else X_t[it]
        lab_t = torch.as_tensor(labels)
        sub_labels = lab_t[torch.as_tensor(idx, device=lab_t.device)]
        sub_w = None
        if weights is not None:
            w_t = to_torch(weights)
            sub_w = w_t[torch.as_tensor(idx, device=w_t.device)]
        coefficients = _silhouette(sub_X, sub_labels, sub_w, metric, device, warn)
    score = _mean(coefficients)
    if input_is_numpy:
        return score.detach().cpu().numpy().item()
    return score
