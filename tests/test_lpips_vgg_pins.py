"""LPIPS-VGG pinned to pyiqa (the reference's `-qm lpips-vgg`, utils/eval_metrics.py:110-147) where pyiqa and its weights exist:
the oracle (CPU) and the kernels (`-m gpu`) against pyiqa.create_metric('lpips-vgg') called as the reference calls it (a gray
frame replicated to three channels, eval_utils.py:46-54), on the metric's own state dict.  The module skips where pyiqa is
missing or cannot load its weights (it downloads them), and until it has run the parity with pyiqa is unpinned: the state-dict
names net.slice1.{0,2} ... net.slice5.{24,26,28} and lin{0..4}.model.1.weight, the pool positions, the shift and scale constants
and the eps of the normalisation.  A convention it contradicts is fixed in tests/lpips_vgg_ref.py and csrc/lpips_vgg.hip together."""
import numpy as np
import pytest

import lpips_vgg_ref as R

pyiqa = pytest.importorskip('pyiqa')

TOL = 2e-4      # relative (+ 1e-7): this project's LPIPS gate; pyiqa computes in fp32 tensors


@pytest.fixture(scope='module')
def metric():
    try:
        return pyiqa.create_metric('lpips-vgg', device='cpu')
    except Exception as e:      # no network, no cached weights
        pytest.skip(f"pyiqa cannot create lpips-vgg here: {e}")


def _pairs():
    img, ref = R.frame_pairs(64, 80)
    return img, ref


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
    for name, shape in weights.lpips_vgg_schema().items():
        assert name in sd and int(np.prod(sd[name].shape)) == int(np.prod(shape)), name


def test_oracle_matches_pyiqa(metric):
    img, ref = _pairs()
    want = _pyiqa_scores(metric, img, ref)
    got, _ = R.lpips_vgg(_state_dict(metric), img, ref)
    assert (np.abs(got - want) <= TOL * np.abs(want) + 1e-7).all(), (got, want)


@pytest.mark.gpu
def test_kernels_match_pyiqa(metric):
    import torch
    from evreal_amd.lpips import LPIPSVGG
    img, ref = _pairs()
    want = _pyiqa_scores(metric, img, ref)
    got = LPIPSVGG(_state_dict(metric))(torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()).cpu().numpy()
    assert (np.abs(got - want) <= TOL * np.abs(want) + 1e-7).all(), (got, want)
