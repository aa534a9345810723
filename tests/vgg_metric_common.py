"""What tests/test_gpu_lpips_vgg.py and tests/test_gpu_dists.py share: the two metrics run on one VGG-16 trunk and through one tracker
path, so their tests feed the same frames and apply the same gate.  Helpers only; every test stays in its metric's file."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bound(want64, want32, scale=1.0):
    """The gate of both metrics: this project's own LPIPS gate (2e-4 relative + 1e-7), or eight times the reference arithmetic's own
    fp32-against-fp64 error on the same inputs where that is larger (the margin rule of tests/test_gpu_wino.py)."""
    return scale * np.maximum(2e-4 * np.abs(want64) + 1e-7, 8.0 * np.abs(want32 - want64))


def run_child(child, mode):
    """`child` (a script that takes the repository root and tests/ as arguments and prints 'RESULT ' + json) in a fresh process with
    EVR_ARITH=mode -- the library reads it once -- -> the decoded result."""
    env = dict(os.environ, EVR_ARITH=mode)
    env.pop('EVR_FP32', None)
    r = subprocess.run([sys.executable, '-c', child, ROOT, os.path.join(ROOT, 'tests')], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])


def write_weights_file(tmp_path, monkeypatch, sd, file, env, cache):
    """The body of a `weights_file` fixture: `sd` saved as tmp_path/file, $env pointing at it, the tracker's handle cache emptied."""
    from evreal_amd import eval_metrics as em
    path = str(tmp_path / file)
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    monkeypatch.setenv(env, path)
    monkeypatch.setattr(em.EvalMetricsTracker, cache, [False, None])
    return path


def _frames(H, W, n):
    rng = np.random.default_rng([H, W, n])
    yy, xx = np.mgrid[0:H, 0:W]
    refs = [(0.5 + 0.4 * np.sin(xx / (5.0 + i)) * np.cos(yy / (6.0 + i))).astype(np.float32) for i in range(n)]
    frames = [(r + 0.2 * rng.standard_normal(r.shape)).astype(np.float32) for r in refs]      # leaves [0,1]: the clip is exercised
    return frames, refs


BATCHES = (3, 5, 2)


def _feed(t, frames, refs):
    idx, k = list(range(len(frames))), 0
    for n in BATCHES:
        t.update_batch(idx[k:k + n], _cuda(np.stack(frames[k:k + n])), _cuda(np.stack(refs[k:k + n])),
                       [0.01 * i for i in idx[k:k + n]], None)
        k += n
    t.finalize(idx[-1])
    return idx
