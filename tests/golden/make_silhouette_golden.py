"""Generate tests/golden/silhouette.npz and tests/golden/silhouette_signatures.json by IMPORTING THE REAL REFERENCE
(TorchDR at /root/reference, CPU ``backend=None``), as make_golden.py does.

    python tests/golden/make_silhouette_golden.py

The npz is written with fixed zip timestamps, so a second run reproduces the same bytes.
"""

import inspect
import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

from torchdr.distance import pairwise_distances  # noqa: E402
from torchdr.eval import silhouette_samples, silhouette_score  # noqa: E402


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


def inputs():
    g = np.random.default_rng(20261016)
    n, d = 300, 5
    centers = g.normal(size=(4, d)) * 2.0
    lab = g.integers(0, 4, size=n)
    X = centers[lab] + 0.7 * g.normal(size=(n, d))
    vals = np.array([-3, 0, 7, 2])
    lab_int = vals[lab].astype(np.int64)
    lab_int[17] = 100      # a singleton
    lab_float = lab_int.astype(np.float64) * 0.5 + 0.25
    Xd = np.sqrt(((X[:120, None, :] - X[None, :120, :]) ** 2).sum(-1))
    Id = np.eye(10)
    y_I = np.arange(10, dtype=np.int64)
    y_I2 = np.repeat(np.arange(5, dtype=np.int64), 2)
    CI = np.sqrt(((Id[:, None, :] - Id[None, :, :]) ** 2).sum(-1))
    return dict(X=X, lab_int=lab_int, lab_float=lab_float, lab_one=np.zeros(n, dtype=np.int64), Xd=Xd,
                lab_d=lab_int[:120].copy(), Id=Id, y_I=y_I, y_I2=y_I2, CI=CI, w_Id=np.full(10, 0.1))


# Weighted input is recorded on equal-sized clusters only: the reference's weighted inter-cluster step fails when two
# clusters differ in size (its prod_matrix_vector scales rows, not columns).
# name: (X key, labels key, weights key or None, metric, sample_size, random_state)
CASES = {
    "eu_int": ("X", "lab_int", None, "euclidean", None, None),
    "l1_int": ("X", "lab_int", None, "manhattan", None, None),
    "eu_float": ("X", "lab_float", None, "euclidean", None, None),
    "eu_one": ("X", "lab_one", None, "euclidean", None, None),
    "eu_sample": ("X", "lab_int", None, "euclidean", 100, 7),
    "l1_sample": ("X", "lab_float", None, "manhattan", 150, 3),
    "pre_int": ("Xd", "lab_d", None, "precomputed", None, None),
    "pre_sample": ("Xd", "lab_d", None, "precomputed", 50, 11),
    "id_eu": ("Id", "y_I", None, "euclidean", None, None),
    "id_l1": ("Id", "y_I", None, "manhattan", None, None),
    "id_pre": ("CI", "y_I", None, "precomputed", None, None),
    "id2_eu": ("Id", "y_I2", None, "euclidean", None, None),
    "id2_eu_w": ("Id", "y_I2", "w_Id", "euclidean", None, None),
    "id2_l1": ("Id", "y_I2", None, "manhattan", None, None),
    "id2_pre": ("CI", "y_I2", None, "precomputed", None, None),
}


def main():
    torch.set_num_threads(4)
    inp = inputs()
    out = {k: v for k, v in inp.items()}
    for name, (xk, lk, wk, metric, ss, rs) in CASES.items():
        for tag, dt in (("32", np.float32), ("64", np.float64)):
            X = inp[xk].astype(dt)
            w = None if wk is None else inp[wk].astype(dt)
            lab = inp[lk]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                if ss is None:
                    s = silhouette_samples(torch.from_numpy(X), torch.from_numpy(lab),
                                           None if w is None else torch.from_numpy(w), metric, None, None, False)
                    out[f"{name}_s{tag}"] = s.numpy()
                score = silhouette_score(X, lab, w, metric, None, None, ss, rs, False)
            out[f"{name}_score{tag}"] = np.float64(score)
            # the reference's own self-distance (its Gram form leaves d_ii != 0; the HIP path has d_ii = 0 exactly)
            if metric != "precomputed":
                C = pairwise_distances(torch.from_numpy(X), torch.from_numpy(X), metric=metric, backend=None)
                out[f"{name}_selfdist{tag}"] = np.float64(C.diagonal().abs().max())
    out["cases"] = np.array(json.dumps(CASES, sort_keys=True))
    path = os.path.join(HERE, "silhouette.npz")
    save_npz(path, out)
    print(f"silhouette: {os.path.getsize(path) / 1024:.0f} KiB")

    def sig(obj):
        ps = inspect.signature(obj).parameters
        return [[k, None if v.default is inspect._empty else repr(v.default)] for k, v in ps.items()]

    sigs = {"eval.silhouette_samples": sig(silhouette_samples), "eval.silhouette_score": sig(silhouette_score)}
    with open(os.path.join(HERE, "silhouette_signatures.json"), "w") as f:
        json.dump(sigs, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
