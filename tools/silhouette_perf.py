"""Time of the exact silhouette (silhouette_samples, euclidean, direct path) on one GPU, from device events:
python tools/silhouette_perf.py [--quick]  -> one JSON line per (N, D, L, dtype).

Every pair costs one distance of D coordinates: 3 flop per coordinate (difference, multiply, add) on the vector ALUs;
`share` is that rate against the dense vector peak of the dtype (MI355X datasheet: 157.3 TFLOP/s fp32, 78.6 TFLOP/s fp64).
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from torchdr_amd.eval.silhouette import _silhouette

PEAK = {torch.float32: 157.3e12, torch.float64: 78.6e12}


def run(n, d, L, dtype, reps):
    g = torch.Generator().manual_seed(n + d + L)
    lab = torch.randint(0, L, (n,), generator=g)
    centers = torch.randn(L, d, generator=g) * 2.0
    X = (centers[lab] + 0.5 * torch.randn(n, d, generator=g)).to("cuda", dtype)
    lab = lab.cuda()
    _silhouette(X, lab, None, "euclidean", None, False)   # warm-up (and module load)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        _silhouette(X, lab, None, "euclidean", None, False)
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) / 1000.0 / reps
    pairs = float(n) * n
    flops = 3.0 * pairs * d
    return {"n": n, "d": d, "L": L, "dtype": str(dtype).replace("torch.", ""), "seconds": round(sec, 5),
            "pairs_per_s": float(f"{pairs / sec:.4g}"), "share_of_vector_peak": round(flops / sec / PEAK[dtype], 4),
            "reps": reps}


def main():
    quick = "--quick" in sys.argv
    sizes = (100_000,) if quick else (100_000, 1_000_000)
    for n in sizes:
        for d in (2, 128):
            for L in (10, 1000):
                for dtype in (torch.float32, torch.float64):
                    reps = 3 if n <= 100_000 else 1
                    t = time.time()
                    out = run(n, d, L, dtype, reps)
                    out["wall_s"] = round(time.time() - t, 2)
                    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
