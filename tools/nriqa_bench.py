"""No-reference IQA kernel timing: evr_niqe_score or evr_brisque_score on n = 1 / 8 / 64 frames of 346x260 and 640x480,
device events around 50 calls after a warm-up; prints one JSON line (microseconds per call and per frame, and the
algorithmic bytes per frame).  With --evaluate it times evaluate() instead: a frame-less synthetic dataset (8 sequences x
160 windows of 15000 events, 346x260, synthetic E2VID weights) with no metric, -qm niqe, -qm brisque and -qm brisque niqe (synthetic models).

    python tools/nriqa_bench.py [--metric niqe|brisque] [--iters 50]
    python tools/nriqa_bench.py --evaluate
"""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(H, W, metric='niqe'):
    """niqe: fp32 frame read once + the fp64 half-size image written and read once + features / score written.
    brisque: fp32 frame read once + the fp64 half-size image written and read once + 2 x 26 tile sums per tile written
    and read once + the score written."""
    if metric == 'brisque':
        Hh, Wh = (H + 1) // 2, (W + 1) // 2
        tiles = -(-H // 32) * -(-W // 32) + -(-Hh // 32) * -(-Wh // 32)
        return 4 * H * W + 2 * 8 * Hh * Wh + 2 * 8 * 26 * tiles + 8
    Hc, Wc = H // 96 * 96, W // 96 * 96
    nb = (Hc // 96) * (Wc // 96)
    return 4 * H * W + 2 * 8 * (Hc // 2) * (Wc // 2) + 8 * nb * 36 + 8


def niqe_model():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((36, 36)) * 0.05
    return dict(mu=np.full(36, 0.5), cov=A @ A.T + 0.01 * np.eye(36), source='synthetic')


def brisque_model(nsv=774):
    """A synthetic SVR of the release's size (774 support vectors), features scaled from [0, 1] to [-1, 1]."""
    rng = np.random.default_rng(0)
    return dict(sv=rng.uniform(-1, 1, (nsv, 36)), coef=rng.standard_normal(nsv), gamma=0.05, rho=-0.5,
                fmin=np.zeros(36), fmax=np.full(36, 10.0), lower=-1.0, upper=1.0, source='synthetic')


def kernels(metric, iters):
    from evreal_amd.nriqa import BRISQUE, NIQE
    m = NIQE(niqe_model()) if metric == 'niqe' else BRISQUE(brisque_model())
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
            for _ in range(iters):
                m(x, out=out)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / iters * 1e3
            res[f'{W}x{H}_n{n}'] = dict(us_per_call=round(us, 1), us_per_frame=round(us / n, 2),
                                        finite=int(torch.isfinite(out).sum()))
        res[f'{W}x{H}_bytes_per_frame'] = algorithmic_bytes(H, W, metric)
    return {metric: res}


def evaluate_rates(reps=3):
    from evreal_amd import eval as ev, synth, weights
    from evreal_amd.nriqa import save_brisque_model, save_niqe_model
    from evreal_amd.eval_metrics import EvalMetricsTracker
    n_seq, frames, W_, H_ = 8, 160, 346, 260
    kw = dict(weights.E2VID_KWARGS)
    sd = weights.synth_state_dict(weights.unet_recurrent_schema(**kw), seed=0)
    tmp = tempfile.mkdtemp(prefix='evr_nriqa_')
    for sub in ('eval', 'method', 'dataset'):
        os.makedirs(os.path.join(tmp, 'config', sub))
    os.makedirs(os.path.join(tmp, 'pretrained'))
    nm, bm = niqe_model(), brisque_model()
    save_niqe_model(os.path.join(tmp, 'pretrained', 'niqe_model.npz'), nm['mu'], nm['cov'], nm['source'])
    save_brisque_model(os.path.join(tmp, 'pretrained', 'brisque_model.npz'),
                       *(bm[k] for k in ('sv', 'coef', 'gamma', 'rho', 'fmin', 'fmax', 'lower', 'upper')), bm['source'])
    torch.save({'model': {k: v for k, v in kw.items() if k != 'final_activation'},
                'state_dict': {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, os.path.join(tmp, 'e2vid.pth'))
    json.dump({"model_name": "E2VID", "model_path": os.path.join(tmp, 'e2vid.pth'), "event_tensor_normalization": True,
               "post_process_norm": "robust"}, open(os.path.join(tmp, 'config', 'method', 'E2VID.json'), 'w'))
    # (no frames to voxelize between: windows of 15000 events)
    json.dump({"dataset_kwargs": {"num_bins": 5, "voxel_method": {"method": "k_events", "k": 15000, "sliding_window_w": 0},
                                  "keep_ratio": 1.0},
               "save_images": False, "histeq": "none", "eval_infer_all": False, "ts_tol_ms": 1.0, "create_video": False,
               "batch_sequences": n_seq}, open(os.path.join(tmp, 'config', 'eval', 'std.json'), 'w'))
    seqs = {}
    for s in range(n_seq):
        synth.write_sequence(os.path.join(tmp, 'data', 'NR', f's{s}'), 100 + s, (frames + 1) * 15000, 1.0e6, W_, H_,
                             1.0e6 / 15000, with_images=False)
        seqs[f's{s}'] = {}
    json.dump({"root_path": os.path.join(tmp, 'data', 'NR'), "sequences": seqs},
              open(os.path.join(tmp, 'config', 'dataset', 'NR.json'), 'w'))
    cwd = os.getcwd()
    os.chdir(tmp)
    res, n_frames = {}, 0
    try:
        # (the frames are counted from the first run's timestamps.txt: a run without metrics may write none)
        for qm in (['niqe'], [], ['brisque'], ['brisque', 'niqe']):
            best = None
            for _ in range(reps):
                shutil.rmtree('outputs', ignore_errors=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    ev.evaluate(['E2VID'], ['std'], ['NR'], qm)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
                if not n_frames:
                    n_frames = sum(len(open(os.path.join('outputs', 'std', 'NR', f's{s}', 'E2VID', 'timestamps.txt')).readlines())
                                   for s in range(n_seq))
            res['-qm ' + (' '.join(qm) or '(none)')] = dict(seconds=round(best, 3), frames=n_frames,
                                                            frames_per_s=round(n_frames / best, 1))
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)
    return dict(evaluate=dict(sequences=n_seq, frames_per_sequence=frames, size=f'{W_}x{H_}', best_of=reps, runs=res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--metric', choices=('niqe', 'brisque'), default='niqe')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--evaluate', action='store_true', help='time evaluate() with and without the no-reference metrics')
    a = ap.parse_args()
    print(json.dumps(evaluate_rates() if a.evaluate else kernels(a.metric, a.iters)))


if __name__ == '__main__':
    main()
