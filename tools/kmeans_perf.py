"""Time of kmeans_ari and of its assignment kernel on one GPU, from device events:
python tools/kmeans_perf.py [--quick] [--out FILE]  -> one JSON line per (N, D, C), also appended to FILE.

* ``assign_ms``: tdr_kmeans_assign_f32 on (N rows, C centres), against ``knn1_ms``, the exact k = 1 search
  (knn_packed / _knn_wide, sqeuclidean) on the same packed inputs; ``tflops`` = 2 N C D / time against the 155 TFLOP/s
  measured fp32 matrix peak (``share``).
* ``call_ms``: the whole kmeans_ari call (20 iterations, nredo = 1) on a mixture of C groups, one timed call after a
  warm-up call.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from torchdr_amd import kmeans_ari
from torchdr_amd.distance.base import PackedPoints, WidePackedPoints, _knn_wide, knn_packed
from torchdr_amd.eval import kmeans as K

PEAK = 155e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(n, d, c, reps, call):
    g = torch.Generator().manual_seed(n + d + c)
    centers = torch.randn(c, d, generator=g) * 2.0
    lab = torch.arange(n) % c
    X = (centers[lab] + 0.5 * torch.randn(n, d, generator=g)).to("cuda")
    C = X[torch.randperm(n, generator=g)[:c].cuda()].contiguous()
    xp, cp = K.pack(X), K.pack(C)
    t_assign = timed(lambda: K.assign(xp, n, C, cp=cp), reps)
    if d > 256:
        t_knn = timed(lambda: _knn_wide(X, C, 1, "sqeuclidean", False), reps)
        pack_ms = timed(lambda: (WidePackedPoints(X), WidePackedPoints(C)), reps)  # _knn_wide packs inside
        t_knn -= pack_ms
    else:
        P, Q = PackedPoints(X), PackedPoints(C)
        t_knn = timed(lambda: knn_packed(P, Q, 1, "sqeuclidean", False), reps)
    flops = 2.0 * n * c * d
    out = {"n": n, "d": d, "c": c, "assign_ms": round(t_assign, 4), "knn1_ms": round(t_knn, 4),
           "assign_over_knn1": round(t_assign / t_knn, 3), "tflops": round(flops / t_assign / 1e9, 2),
           "share": round(flops / (t_assign / 1e3) / PEAK, 4), "reps": reps}
    if call:
        y = lab.cuda()
        kmeans_ari(X, y, n_clusters=c, random_state=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kmeans_ari(X, y, n_clusters=c, random_state=0)
        torch.cuda.synchronize()
        out["call_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    return out


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    sizes = (100_000,) if quick else (100_000, 1_000_000)
    for n in sizes:
        for d in (16, 128, 784):
            for c in (10, 100, 1000, 4096):
                reps = 5 if n * c * d <= 1e11 else 2
                out = run(n, d, c, reps, call=True)
                line = json.dumps(out)
                print(line, flush=True)
                if path:
                    with open(path, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
