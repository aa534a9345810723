"""BRISQUE pinned to pyiqa (the reference's `-qm brisque`, utils/eval_metrics.py:110-147) where pyiqa, its weights and the
MATLAB release's libsvm model with its range file exist: the oracle (CPU) and the kernels (`-m gpu`) against
pyiqa.create_metric('brisque') called as the reference calls it (a gray frame replicated to three channels,
eval_utils.py:46-54).  Skips where any of them is missing.  A convention it contradicts (input rounding, padding, the
text round trips) is fixed in tests/brisque_ref.py and csrc/nriqa.hip together."""

import numpy as np
import pytest

import brisque_ref as B


def _setup():
    pyiqa = pytest.importorskip('pyiqa')
    from evreal_amd.eval_metrics import brisque_model_path
    from evreal_amd.nriqa import load_brisque_model
    found = brisque_model_path()
    if found is None or found[1] is None:
        pytest.skip("no libsvm BRISQUE model with its range file ($EVREAL_BRISQUE_MODEL or pretrained/allmodel + allrange)")
    import torch
    metric = pyiqa.create_metric('brisque', device='cpu')
    return torch, metric, load_brisque_model(*found)


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
        got = B.brisque(v, model)
        assert abs(got - want) <= 1e-4 * max(abs(want), 1.0), (got, want)


@pytest.mark.gpu
def test_kernel_matches_pyiqa():
    torch, metric, model = _setup()
    from evreal_amd.nriqa import BRISQUE
    frames = _frames()
    got = BRISQUE(model)(torch.from_numpy(np.stack(frames)).cuda()).cpu().numpy()
    for g, v in zip(got, frames):
        want = _pyiqa(torch, metric, v)
        assert abs(g - want) <= 1e-4 * max(abs(want), 1.0), (g, want)
