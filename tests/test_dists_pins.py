"""DISTS pinned to pyiqa (the reference's `-qm dists`, utils/eval_metrics.py:110-147) where pyiqa and its weights exist: the oracle
(CPU) and the kernels (`-m gpu`) against pyiqa.create_metric('dists') called as the reference calls it (a gray frame replicated
to three channels, eval_utils.py:46-54), on the metric's own state dict.  The module skips where pyiqa is missing or cannot load
its weights (it downloads them), and until it has run the parity with pyiqa is unpinned: the state-dict names stage1.{0,2} ...
stage5.{24,26,28}, alpha, beta, mean and std, the L2 pool (its filter, padding and 1e-12), the mean / std constants, c1 = c2 = 1e-6,
the two-pass variance and the score 1 - (D1 + D2).  A convention it contradicts is fixed in tests/dists_ref.py and csrc/dists.hip
together."""
import numpy as np
import pytest

import dists_ref as R

pyiqa = pytest.importorskip('pyiqa')

TOL = 2e-4      # relative (+ 1e-7): this project's LPIPS gate; pyiqa computes in fp32 tensors


@pytest.fixture(scope='module')
def metric():
    try:
        return pyiqa.create_metric('dists', device='cpu')
    except Exception as e:      # no network, no cached weights
        pytest.skip(f"pyiqa cannot create dists here: {e}")


def _pyiqa_scores(metric, img, ref):
    import torch
    rgb = lambda v: torch.from_numpy(v).unsqueeze(1).repeat(1, 3, 1, 1)
    with torch.no_grad():
        return metric(rgb(img), rgb(ref)).reshape(-1).double().numpy()


def _state_dict(metric):
    return {k: v.detach().cpu().numpy() for k, v in metric.net.state_dict().items()}


def test_state_dict_has_the_schema_names(metric):
    from evreal_amd import weights
    sd = _state_dict(metric)
    for name, shape in weights.dists_schema().items():
        assert name in sd and int(np.prod(sd[name].shape)) == int(np.prod(shape)), name
    assert (sd['alpha'] > 0).all() and (sd['beta'] > 0).all()
    for name, want in (('mean', R.MEAN), ('std', R.STD)):      # optional buffers: where present they hold the constants
        if name in sd:
            np.testing.assert_allclose(sd[name].reshape(-1), want, rtol=0, atol=1e-6)
    rest = [k for k in sd if k not in weights.dists_schema() and k not in ('mean', 'std')]
    assert all(k.endswith('.filter') for k in rest), rest      # the pools' buffers: ignored by evr_dists_create


def test_oracle_matches_pyiqa(metric):
    img, ref = R.frame_pairs(64, 80)
    want = _pyiqa_scores(metric, img, ref)
    got, _ = R.dists(_state_dict(metric), img, ref)
    assert (np.abs(got - want) <= TOL * np.abs(want) + 1e-7).all(), (got, want)


@pytest.mark.gpu
def test_kernels_match_pyiqa(metric):
    import torch
    from evreal_amd.lpips import DISTS
    img, ref = R.frame_pairs(64, 80)
    want = _pyiqa_scores(metric, img, ref)
    got = DISTS(_state_dict(metric))(torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()).cpu().numpy()
    assert (np.abs(got - want) <= TOL * np.abs(want) + 1e-7).all(), (got, want)
