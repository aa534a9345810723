"""NIQE kernel timing: evr_niqe_score on n = 1 / 8 / 64 frames of 346x260 and 640x480, device events around 50 calls after
a warm-up; prints one JSON line (microseconds per call and per frame, and the algorithmic bytes per frame).

    python tools/nriqa_bench.py [--iters 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def algorithmic_bytes(H, W):
    """fp32 frame read once + the fp64 half-size image written and read once + features / score written."""
    Hc, Wc = H // 96 * 96, W // 96 * 96
    nb = (Hc // 96) * (Wc // 96)
    return 4 * H * W + 2 * 8 * (Hc // 2) * (Wc // 2) + 8 * nb * 36 + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    from evreal_amd.nriqa import NIQE
    rng = np.random.default_rng(0)
    A = rng.standard_normal((36, 36)) * 0.05
    m = NIQE(dict(mu=np.full(36, 0.5), cov=A @ A.T + 0.01 * np.eye(36)))
    res = {}
    for H, W in ((260, 346), (480, 640)):
        for n in (1, 8, 64):
            x = torch.rand((n, H, W), device='cuda')
            out = torch.empty(n, dtype=torch.float64, device='cuda')
            for _ in range(5):
                m(x, out=out)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                m(x, out=out)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / a.iters * 1e3
            res[f'{W}x{H}_n{n}'] = dict(us_per_call=round(us, 1), us_per_frame=round(us / n, 2),
                                        finite=int(torch.isfinite(out).sum()))
        res[f'{W}x{H}_bytes_per_frame'] = algorithmic_bytes(H, W)
    print(json.dumps(dict(niqe=res)))


if __name__ == '__main__':
    main()
