"""NIQE pinned to pyiqa (the reference's `-qm niqe`, utils/eval_metrics.py:110-147) where pyiqa and the MATLAB model file
exist: the oracle (CPU) and the kernels (`-m gpu`) against pyiqa.create_metric('niqe') called as the reference calls it (a
gray frame replicated to three channels, eval_utils.py:46-54).  Skips where either is missing.  A convention it contradicts
(input rounding, padding, NaN handling) is fixed in tests/nriqa_ref.py and csrc/nriqa.hip together."""

import numpy as np
import pytest

import nriqa_ref as R


def _setup():
    pyiqa = pytest.importorskip('pyiqa')
    from evreal_amd.eval_metrics import niqe_model_path
    from evreal_amd.nriqa import load_niqe_model
    path = niqe_model_path()
    if path is None or not path.endswith('.mat'):
        pytest.skip("no niqe_modelparameters.mat ($EVREAL_NIQE_MODEL or pretrained/)")
    import torch
    metric = pyiqa.create_metric('niqe', device='cpu')
    return torch, metric, load_niqe_model(path)


def _frames():
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:260, 0:346].astype(np.float64)
    out = []
    for k in range(3):
        a = 0.5 + 0.3 * np.sin(xx / (6.0 + k)) * np.cos(yy / 9.0) + 0.1 * rng.standard_normal((260, 346))
        out.append(np.clip(a, 0, 1).astype(np.float32))
    return out


def _pyiqa(torch, metric, v):
    t = torch.from_numpy(v)[None].repeat(3, 1, 1)[None]
    return float(metric(t).squeeze())


def test_oracle_matches_pyiqa():
    torch, metric, model = _setup()
    for v in _frames():
        want = _pyiqa(torch, metric, v)
        got = R.niqe(v, model['mu'], model['cov'])
        assert abs(got - want) <= 1e-4 * abs(want), (got, want)


@pytest.mark.gpu
def test_kernel_matches_pyiqa():
    torch, metric, model = _setup()
    from evreal_amd.nriqa import NIQE
    frames = _frames()
    got = NIQE(model)(torch.from_numpy(np.stack(frames)).cuda()).cpu().numpy()
    for g, v in zip(got, frames):
        want = _pyiqa(torch, metric, v)
        assert abs(g - want) <= 1e-4 * abs(want), (g, want)
