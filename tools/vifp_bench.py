"""VIFp kernel timing: evr_vifp beside evr_fr_metrics with ms_ssim (the nearest existing kernel: a Gaussian pyramid in fp64) on
the same 16 frame pairs of 346x260, 640x480 and 970x624 -- device events around `--iters` calls of each, alternating, `--reps`
times after a warm-up.  One process per shape, each under its own time limit (tools/metric_bench.py).  Prints one JSON line and
writes it to --out: microseconds per call and per frame of both (the best and every repeat), their ratio, and the fraction of
VIFp's read floor (8 H W algorithmic bytes per frame at the 8.0 TB/s HBM peak) its time stands for.

    python tools/vifp_bench.py [--frames 16] [--iters 200] [--reps 5] [--out profiles/vifp_bench.json]
"""
import metric_bench as mb


def run_shape(a, H, W):
    import torch
    from evreal_amd.prepost import VIFP, FullRefMetrics
    vifp, fr, n = VIFP(), FullRefMetrics(), a.frames
    img, ref = mb.pairs(n, H, W)
    vo = torch.empty((n, 9), dtype=torch.float64, device='cuda')
    mo = torch.empty((n, 2), dtype=torch.float64, device='cuda')
    runs = {'vifp': lambda: vifp.stats(img, ref, out=vo), 'ms_ssim': lambda: fr(img, ref, psnr=False, ms_ssim=True, out=mo)}
    best, entry = mb.entries(mb.alternate(runs, a.iters, a.reps), n)
    return dict(entry, vifp_over_ms_ssim=round(best['vifp'] / best['ms_ssim'], 3), **mb.read_floor(best['vifp'], n, H, W),
                mean_score=round(float(vo[:, 0].mean()), 5), mean_ms_ssim=round(float(mo[:, 1].mean()), 5),
                finite=[int(torch.isfinite(vo).all()), int(torch.isfinite(mo).all())])


def main():
    a = mb.parser(frames=16, iters=200, reps=5).parse_args()
    mb.run(__file__, a, run_shape, lambda res: dict(frames=a.frames, iters=a.iters, reps=a.reps, hbm_peak_bytes_per_s=mb.HBM_PEAK,
                                                     launches_per_call=dict(vifp=5, ms_ssim=6), shapes=res))


if __name__ == '__main__':
    main()
