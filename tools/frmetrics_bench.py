"""Full-reference metric kernel timing: evr_fr_metrics (PSNR + MS-SSIM, fp64) beside evr_metrics (MSE + SSIM) on the same 512
frame pairs of 346x260 in the same run -- device events around `--iters` calls of each after a warm-up, in a child process under
a time limit (tools/metric_bench.py); prints one JSON line (microseconds per call and per frame, the algorithmic bytes per frame
of both, and their ratios).  Under `rocprofv3 --kernel-trace --stats` a `--shape 260x346` run gives the per-kernel table of
profiles/frmetrics_kernel_stats.md.
With --evaluate it times evaluate() instead: a synthetic dataset with frames (8 sequences x 160 windows between frames, 346x260,
synthetic E2VID weights) with -qm mse ssim and -qm mse ssim psnr ms_ssim, alternating, three times each.

    python tools/frmetrics_bench.py [--frames 512] [--iters 10]
    python tools/frmetrics_bench.py --evaluate
"""
import contextlib
import io
import json
import os
import shutil
import tempfile
import time

import numpy as np
import torch

import metric_bench as mb


def level_sizes(H, W):
    out = [(H, W)]
    for _ in range(4):
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


def algorithmic_bytes(H, W):
    """evr_metrics: both fp32 frames read once.  evr_fr_metrics: the same, plus the four pooled levels of both images written
    once and read once in fp64 (partial sums and scores are a few hundred bytes)."""
    base = 2 * 4 * H * W
    return base, base + sum(2 * 2 * 8 * h * w for h, w in level_sizes(H, W)[1:])


def run_shape(a, H, W):
    from evreal_amd.prepost import FullRefMetrics, Metrics
    n = a.frames
    ref = torch.rand((n, H, W), device='cuda')
    img = (ref + 0.06 * torch.randn((n, H, W), device='cuda')).contiguous()
    old, new = Metrics(), FullRefMetrics()
    out = torch.empty((n, 2), dtype=torch.float64, device='cuda')
    runs = {'evr_metrics (mse + ssim)': lambda: old(img, ref),
            'evr_fr_metrics (psnr + ms_ssim)': lambda: new(img, ref, out=out),
            'evr_fr_metrics (psnr alone)': lambda: new(img, ref, ms_ssim=False, out=out)}
    best, res = mb.entries(mb.alternate(runs, a.iters, 1, warmup=3), n, repeats=False, digits=3)
    b_old, b_new = algorithmic_bytes(H, W)
    t_old, t_new = res['evr_metrics (mse + ssim)']['us_per_call'], res['evr_fr_metrics (psnr + ms_ssim)']['us_per_call']
    return dict(size=f'{W}x{H}', frames=n, iters=a.iters, runs=res, bytes_per_frame=dict(evr_metrics=b_old, evr_fr_metrics=b_new),
                bytes_ratio=round(b_new / b_old, 3), time_ratio=round(t_new / t_old, 3),
                finite=int(torch.isfinite(out).all()))


def evaluate_rates(reps=3):
    from evreal_amd import eval as ev, synth, weights
    n_seq, frames, W_, H_ = 8, 160, 346, 260
    kw = dict(weights.E2VID_KWARGS)
    sd = weights.synth_state_dict(weights.unet_recurrent_schema(**kw), seed=0)
    tmp = tempfile.mkdtemp(prefix='evr_fr_')
    for sub in ('eval', 'method', 'dataset'):
        os.makedirs(os.path.join(tmp, 'config', sub))
    torch.save({'model': {k: v for k, v in kw.items() if k != 'final_activation'},
                'state_dict': {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, os.path.join(tmp, 'e2vid.pth'))
    json.dump({"model_name": "E2VID", "model_path": os.path.join(tmp, 'e2vid.pth'), "event_tensor_normalization": True,
               "post_process_norm": "robust"}, open(os.path.join(tmp, 'config', 'method', 'E2VID.json'), 'w'))
    json.dump({"dataset_kwargs": {"num_bins": 5, "voxel_method": {"method": "between_frames"}, "keep_ratio": 1.0},
               "save_images": False, "histeq": "none", "eval_infer_all": False, "ts_tol_ms": 1.0, "create_video": False,
               "batch_sequences": n_seq}, open(os.path.join(tmp, 'config', 'eval', 'std.json'), 'w'))
    seqs = {}
    for s in range(n_seq):
        synth.write_sequence(os.path.join(tmp, 'data', 'SYN', f's{s}'), 100 + s, (frames + 1) * 15000, 1.0e6, W_, H_, 1.0e6 / 15000)
        seqs[f's{s}'] = {}
    json.dump({"root_path": os.path.join(tmp, 'data', 'SYN'), "sequences": seqs},
              open(os.path.join(tmp, 'config', 'dataset', 'SYN.json'), 'w'))
    cwd = os.getcwd()
    os.chdir(tmp)
    lists = (['mse', 'ssim'], ['mse', 'ssim', 'psnr', 'ms_ssim'])
    secs, n_frames, scored = {' '.join(q): [] for q in lists}, 0, {}
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ev.evaluate(['E2VID'], ['std'], ['SYN'], lists[0])          # warm-up: model cache, library, allocator
        for _ in range(reps):
            for qm in lists:                                            # alternating
                shutil.rmtree('outputs', ignore_errors=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    ev.evaluate(['E2VID'], ['std'], ['SYN'], qm)
                torch.cuda.synchronize()
                secs[' '.join(qm)].append(time.perf_counter() - t0)
                out = lambda s, f: os.path.join('outputs', 'std', 'SYN', f's{s}', 'E2VID', f + '.txt')
                n_frames = sum(len(open(out(s, 'timestamps')).readlines()) for s in range(n_seq))
                scored[' '.join(qm)] = {m: sum(len(open(out(s, m)).readlines()) for s in range(n_seq)) for m in qm}
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)
    runs = {'-qm ' + k: dict(seconds=[round(x, 3) for x in v], frames=n_frames, lines=scored[k],
                             frames_per_s=[round(n_frames / x, 1) for x in v]) for k, v in secs.items()}
    return dict(evaluate=dict(sequences=n_seq, frames_per_sequence=frames, size=f'{W_}x{H_}', repeats=reps, runs=runs))


def main():
    ap = mb.parser(frames=512, iters=10)
    ap.add_argument('--evaluate', action='store_true', help='time evaluate() with and without psnr / ms_ssim')
    a = ap.parse_args()
    if a.evaluate:
        print(json.dumps(evaluate_rates()))
    else:
        mb.run(__file__, a, run_shape, lambda res: res['346x260'], shapes=((260, 346),))


if __name__ == '__main__':
    main()
