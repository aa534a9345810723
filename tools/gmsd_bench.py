"""GMSD kernel timing: evr_gmsd beside evr_fr_metrics with which = 1 (PSNR alone, which reads the same 2*4*H*W bytes per
frame) on the same 16 frame pairs of 346x260, 640x480 and 970x624 in the same run -- device events around `--iters` calls of
each, alternating, `--reps` times after a warm-up; one process.  Prints one JSON line and writes it to --out: microseconds
per call and per frame of both (the best and every repeat), their ratio, and the fraction of GMSD's read floor (8 H W
algorithmic bytes per frame at the 8.0 TB/s HBM peak) its time stands for.  Under `rocprofv3 --kernel-trace --stats` the same
run gives the per-kernel table of profiles/gmsd_kernel_stats.md.

    python tools/gmsd_bench.py [--frames 16] [--iters 500] [--reps 5] [--out profiles/gmsd_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12           # bytes/s, the part's specification
SHAPES = ((260, 346), (480, 640), (624, 970))


def pairs(n, H, W):
    """A smooth texture in [0, 1] and a copy 6 % of noise away: edges in every tile."""
    g = torch.Generator(device='cuda').manual_seed(H * 1000 + W)
    yy = torch.arange(H, device='cuda', dtype=torch.float32)[:, None]
    xx = torch.arange(W, device='cuda', dtype=torch.float32)[None, :]
    base = 0.5 + 0.25 * torch.sin(xx / 5.0) * torch.cos(yy / 6.0)
    ref = (base[None] + 0.02 * torch.randn((n, H, W), device='cuda', generator=g)).clamp_(0.0, 1.0).contiguous()
    img = (ref + 0.06 * torch.randn((n, H, W), device='cuda', generator=g)).clamp_(0.0, 1.0).contiguous()
    return img, ref


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def run(n, iters, reps):
    from evreal_amd.prepost import GMSD, FullRefMetrics
    gmsd, fr = GMSD(), FullRefMetrics()
    res = {}
    for H, W in SHAPES:
        img, ref = pairs(n, H, W)
        go = torch.empty((n, 2), dtype=torch.float64, device='cuda')
        po = torch.empty((n, 2), dtype=torch.float64, device='cuda')
        qm = torch.empty((n, H // 2, W // 2), dtype=torch.float64, device='cuda')
        runs = {'gmsd': lambda: gmsd.stats(img, ref, out=go), 'psnr': lambda: fr(img, ref, ms_ssim=False, out=po),
                'gmsd_with_map': lambda: gmsd.stats(img, ref, out=go, out_map=qm)}
        for fn in runs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():              # alternating
                us[k].append(timed(fn, iters))
        best = {k: min(v) for k, v in us.items()}
        floor_us = 8 * H * W * n / HBM_PEAK * 1e6
        entry = {k: dict(us_per_call=round(best[k], 1), us_per_frame=round(best[k] / n, 2),
                         repeats_us_per_call=[round(v, 1) for v in us[k]]) for k in runs}
        res[f'{W}x{H}'] = dict(
            entry, gmsd_over_psnr=round(best['gmsd'] / best['psnr'], 3), bytes_per_frame=8 * H * W,
            read_floor_us_per_call=round(floor_us, 3), read_floor_fraction=round(floor_us / best['gmsd'], 4),
            mean_score=round(float(go[:, 0].mean()), 5), mean_psnr=round(float(po[:, 0].mean()), 3),
            finite=[int(torch.isfinite(go).all()), int(torch.isfinite(po).all())])
    return dict(frames=n, iters=iters, reps=reps, hbm_peak_bytes_per_s=HBM_PEAK, launches_per_call=dict(gmsd=2, psnr=2),
                shapes=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--iters', type=int, default=500)
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
