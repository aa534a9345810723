"""DISTS timing: DISTS beside LPIPSVGG (the same thirteen convolutions) on the same 16 frame pairs of 346x260, 640x480 and 970x624 in the
same run -- device events around `--iters` calls of each, alternating, `--reps` times after a warm-up of every shape; one process.
Prints one JSON line and writes it to --out: microseconds per call and per pair of both (the best and every repeat), their ratio,
the algorithmic TFLOP/s of DISTS (evr_dists_flops over its time: the thirteen convolutions, the streaming kernels' time included in
the denominator), and the byte floor of the new streaming kernels (dists_stat_pool_kernel: one read of each stage's features plus one
write of each pooled tensor at 4 B per channel; dists_gray_kernel: one read of both gray frames; dists_channel_kernel: one read of
the partial sums; dists_finish_kernel: one read of the chunk terms -- at the 8.0 TB/s HBM peak).

Their own time comes from a profiler run, one shape at a time, because event timing sees whole calls only:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/dists_bench.py --profile 20 --shapes 346x260
    python tools/dists_bench.py --kernel-stats <dir>/.../*_kernel_stats.csv --profiled-calls 22 --stats-shape 346x260 --out ...

(--profile N makes 2 + N plain calls of DISTS and times nothing; the second command runs the timing of every shape and adds, for the
profiled shape, the kernels' microseconds per call from the table and the fraction of their floor that stands for.)  Without
--kernel-stats, and for the other shapes, the kernel times are reported as "not measured".

    python tools/dists_bench.py [--pairs 16] [--iters 20] [--reps 5] [--out profiles/dists_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lpips_vgg_bench import HBM_PEAK, SHAPES, TAP_C, kernel_table, pairs, timed      # noqa: E402


def stat_blocks(nwin, C):
    """csrc/dists.hip stat_blocks: work-groups per pair of a stage's statistics launch."""
    pw = 1 if C >= 256 else 256 // C
    return max(1, min(256, (nwin + 32 * pw - 1) // (32 * pw)))


def byte_floors(n, H, W):
    """Algorithmic bytes per call of the new kernels (both frames of n pairs, 4 B per channel in every format)."""
    stat_pool, partial, h, w = 0, 0, H, W
    for l, c in enumerate(TAP_C):
        h2, w2 = (h + 1) // 2, (w + 1) // 2
        stat_pool += 2 * n * h * w * c * 4 + (2 * n * h2 * w2 * c * 4 if l < 4 else 0)
        partial += n * stat_blocks(h2 * w2, c) * c * 5 * 8
        h, w = h2, w2
    gray_blocks = max(1, min(32, (H * W + 4095) // 4096))
    return {'dists_stat_pool_kernel': stat_pool, 'dists_gray_kernel': 2 * n * H * W * 4, 'dists_channel_kernel': partial,
            'dists_finish_kernel': n * (23 * 4 + gray_blocks * 5) * 8}


def models():
    from evreal_amd import weights
    from evreal_amd.lpips import DISTS, LPIPSVGG
    return LPIPSVGG(weights.synth_lpips_vgg_state_dict(seed=3)), DISTS(weights.synth_dists_state_dict(seed=3))


def profile(n, calls, shapes):
    _, dists = models()
    for H, W in shapes:
        img, ref = pairs(n, H, W)
        out = torch.empty(n, dtype=torch.float64, device='cuda')
        for _ in range(2 + calls):
            dists(img, ref, out=out)
        torch.cuda.synchronize()
    print(json.dumps(dict(profiled_calls=2 + calls, shapes=[f'{W}x{H}' for H, W in shapes])))


def run(n, iters, reps, shapes, table, profiled_calls, stats_shape):
    vgg, dists = models()
    res = {}
    data = {}
    for H, W in shapes:
        data[(H, W)] = pairs(n, H, W)
    for H, W in shapes:          # (every shape is warmed up before its own windows: buffers, plans, code objects)
        img, ref = data[(H, W)]
        vo = torch.empty(n, dtype=torch.float64, device='cuda')
        do = torch.empty(n, dtype=torch.float64, device='cuda')
        runs = {'dists': lambda: dists(img, ref, out=do), 'lpips_vgg': lambda: vgg(img, ref, out=vo)}
        for fn in runs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():              # alternating
                us[k].append(timed(fn, iters))
        best = {k: min(v) for k, v in us.items()}
        flops = dists.flops()
        entry = {k: dict(us_per_call=round(best[k], 1), us_per_pair=round(best[k] / n, 2),
                         repeats_us_per_call=[round(v, 1) for v in us[k]]) for k in runs}
        kernels = {}
        for name, nbytes in byte_floors(n, H, W).items():
            floor_us = nbytes / HBM_PEAK * 1e6
            k = dict(bytes_per_call=nbytes, floor_us_per_call=round(floor_us, 2), us_per_call='not measured', floor_fraction='not measured')
            if table is not None and stats_shape == f'{W}x{H}':
                ns = sum(v for key, v in table.items() if name in key)
                if ns > 0:
                    k['us_per_call'] = round(ns / profiled_calls / 1e3, 1)
                    k['floor_fraction'] = round(floor_us / (ns / profiled_calls / 1e3), 4)
            kernels[name] = k
        res[f'{W}x{H}'] = dict(
            entry, dists_over_lpips_vgg=round(best['dists'] / best['lpips_vgg'], 3), gflop_per_call=round(flops / 1e9, 2),
            algorithmic_tflops=round(flops / (best['dists'] * 1e-6) / 1e12, 1), kernels=kernels,
            saturation=dists.saturation(), mean_score=round(float(do.mean()), 5), mean_lpips_vgg=round(float(vo.mean()), 5),
            finite=[int(torch.isfinite(do).all()), int(torch.isfinite(vo).all())])
    return dict(pairs=n, iters=iters, reps=reps, arith=os.environ.get('EVR_ARITH', 'h3'), hbm_peak_bytes_per_s=HBM_PEAK, shapes=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', nargs='*', default=None, help='a subset of 346x260 640x480 970x624 (W x H)')
    ap.add_argument('--profile', type=int, default=0, help='make 2 + N plain calls per shape for a profiler and time nothing')
    ap.add_argument('--kernel-stats', default=None, help='rocprofv3 --stats kernel table (csv) of a --profile run of ONE shape')
    ap.add_argument('--stats-shape', default='346x260', help='the shape of that run')
    ap.add_argument('--profiled-calls', type=int, default=0, help='calls of that run (what it printed)')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    shapes = SHAPES if not a.shapes else tuple((int(s.split('x')[1]), int(s.split('x')[0])) for s in a.shapes)
    if a.profile:
        profile(a.pairs, a.profile, shapes)
        return
    table = kernel_table(a.kernel_stats) if a.kernel_stats and a.profiled_calls > 0 else None
    line = json.dumps(run(a.pairs, a.iters, a.reps, shapes, table, a.profiled_calls, a.stats_shape))
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
