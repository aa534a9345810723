"""PIQE kernel timing: evr_piqe_score beside evr_brisque_score (a synthetic 774-vector model) on the same 16 frames of
346x260, 640x480 and 970x624 in the same run -- device events around `--iters` calls of each, alternating, `--reps` times
after a warm-up; one process.  Prints one JSON line and writes it to --out: microseconds per call and per frame of both
(the best and every repeat), their ratio, and the fraction of PIQE's read floor (4 H W algorithmic bytes per frame at the
8.0 TB/s HBM peak) its time stands for.  Under `rocprofv3 --kernel-trace --stats` the same run gives the per-kernel table of
profiles/piqe_kernel_stats.md.

    python tools/piqe_bench.py [--frames 16] [--iters 50] [--reps 5] [--out profiles/piqe_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HBM_PEAK = 8.0e12           # bytes/s, the part's specification
SHAPES = ((260, 346), (480, 640), (624, 970))


def frames(n, H, W):
    """A smooth texture plus noise in [0, 1]: most blocks are active, so every block runs both criteria."""
    g = torch.Generator(device='cuda').manual_seed(H * 1000 + W)
    yy = torch.arange(H, device='cuda', dtype=torch.float32)[:, None]
    xx = torch.arange(W, device='cuda', dtype=torch.float32)[None, :]
    base = 0.5 + 0.25 * torch.sin(xx / 5.0) * torch.cos(yy / 6.0)
    return (base[None] + 0.05 * torch.randn((n, H, W), device='cuda', generator=g)).clamp_(0.0, 1.0).contiguous()


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def run(n, iters, reps):
    from evreal_amd.nriqa import BRISQUE, PIQE
    from nriqa_bench import brisque_model
    piqe, brisque = PIQE(), BRISQUE(brisque_model())
    res = {}
    for H, W in SHAPES:
        x = frames(n, H, W)
        po = torch.empty(n, dtype=torch.float64, device='cuda')
        bo = torch.empty(n, dtype=torch.float64, device='cuda')
        runs = {'piqe': lambda: piqe(x, out=po), 'brisque': lambda: brisque(x, out=bo)}
        for fn in runs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():              # alternating
                us[k].append(timed(fn, iters))
        best = {k: min(v) for k, v in us.items()}
        floor_us = 4 * H * W * n / HBM_PEAK * 1e6
        _, flags = piqe.blocks(x)
        res[f'{W}x{H}'] = dict(
            piqe=dict(us_per_call=round(best['piqe'], 1), us_per_frame=round(best['piqe'] / n, 2),
                      repeats_us_per_call=[round(v, 1) for v in us['piqe']]),
            brisque=dict(us_per_call=round(best['brisque'], 1), us_per_frame=round(best['brisque'] / n, 2),
                         repeats_us_per_call=[round(v, 1) for v in us['brisque']]),
            piqe_over_brisque=round(best['piqe'] / best['brisque'], 3),
            piqe_bytes_per_frame=4 * H * W, read_floor_us_per_call=round(floor_us, 3),
            read_floor_fraction=round(floor_us / best['piqe'], 4),
            active_blocks=round(float((flags & 1).float().mean()), 3), mean_score=round(float(po.mean()), 3),
            finite=[int(torch.isfinite(po).sum()), int(torch.isfinite(bo).sum())])
    return dict(frames=n, iters=iters, reps=reps, hbm_peak_bytes_per_s=HBM_PEAK, launches_per_call=dict(piqe=2, brisque=4),
                shapes=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    line = json.dumps(run(a.frames, a.iters, a.reps))
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
