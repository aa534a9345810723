"""GMSD kernel timing: evr_gmsd beside evr_fr_metrics with which = 1 (PSNR alone, which reads the same 2*4*H*W bytes per
frame) on the same 16 frame pairs of 346x260, 640x480 and 970x624 -- device events around `--iters` calls of each,
alternating, `--reps` times after a warm-up.  One process per shape, each under its own time limit (tools/metric_bench.py).
Prints one JSON line and writes it to --out: microseconds per call and per frame of both (the best and every repeat), their
ratio, and the fraction of GMSD's read floor (8 H W algorithmic bytes per frame at the 8.0 TB/s HBM peak) its time stands for.
Under `rocprofv3 --kernel-trace --stats` a `--shape HxW` run gives the per-kernel table of profiles/gmsd_kernel_stats.md.

    python tools/gmsd_bench.py [--frames 16] [--iters 500] [--reps 5] [--out profiles/gmsd_bench.json]
"""
import metric_bench as mb


def run_shape(a, H, W):
    import torch
    from evreal_amd.prepost import GMSD, FullRefMetrics
    gmsd, fr, n = GMSD(), FullRefMetrics(), a.frames
    img, ref = mb.pairs(n, H, W)
    go = torch.empty((n, 2), dtype=torch.float64, device='cuda')
    po = torch.empty((n, 2), dtype=torch.float64, device='cuda')
    qm = torch.empty((n, H // 2, W // 2), dtype=torch.float64, device='cuda')
    runs = {'gmsd': lambda: gmsd.stats(img, ref, out=go), 'psnr': lambda: fr(img, ref, ms_ssim=False, out=po),
            'gmsd_with_map': lambda: gmsd.stats(img, ref, out=go, out_map=qm)}
    best, entry = mb.entries(mb.alternate(runs, a.iters, a.reps), n)
    return dict(entry, gmsd_over_psnr=round(best['gmsd'] / best['psnr'], 3), **mb.read_floor(best['gmsd'], n, H, W),
                mean_score=round(float(go[:, 0].mean()), 5), mean_psnr=round(float(po[:, 0].mean()), 3),
                finite=[int(torch.isfinite(go).all()), int(torch.isfinite(po).all())])


def main():
    a = mb.parser(frames=16, iters=500, reps=5).parse_args()
    mb.run(__file__, a, run_shape, lambda res: dict(frames=a.frames, iters=a.iters, reps=a.reps, hbm_peak_bytes_per_s=mb.HBM_PEAK,
                                                     launches_per_call=dict(gmsd=2, psnr=2), shapes=res))


if __name__ == '__main__':
    main()
