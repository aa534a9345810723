"""GMSD pinned to pyiqa (the reference's `-qm gmsd`, utils/eval_metrics.py:110-147) where pyiqa exists: the oracle (CPU) and
the kernel (`-m gpu`) against pyiqa.create_metric('gmsd') called as the reference calls it (a gray frame replicated to
three channels, eval_utils.py:46-54).  GMSD has no weights, so pyiqa alone is enough; the module skips where it is missing,
and until it has run the parity with pyiqa is unpinned.  A convention it contradicts (the rounding of the luminance, the
pooling of an odd side, the padding of the gradients, the N - 1 of the deviation) is fixed in tests/gmsd_ref.py and
csrc/gmsd.hip together."""
import pytest

import gmsd_ref as G
from thirdparty_refs import image_pairs

pyiqa = pytest.importorskip('pyiqa')

TOL = 1e-4      # relative: pyiqa computes in fp32 tensors


def _pairs():
    return image_pairs()[:3]


def _pyiqa_metric():
    import torch
    metric = pyiqa.create_metric('gmsd', device='cpu')
    rgb = lambda v: torch.from_numpy(v)[None].repeat(3, 1, 1)[None]
    return lambda img, ref: float(metric(rgb(img), rgb(ref)).squeeze())


def test_oracle_matches_pyiqa():
    ref_fn = _pyiqa_metric()
    for name, img, ref in _pairs():
        got, want = G.gmsd(img, ref), ref_fn(img, ref)
        assert abs(got - want) <= TOL * abs(want), (name, got, want)


@pytest.mark.gpu
def test_kernel_matches_pyiqa():
    import torch
    from evreal_amd.prepost import GMSD
    ref_fn, gm = _pyiqa_metric(), GMSD()
    for name, img, ref in _pairs():
        got = float(gm(torch.from_numpy(img[None]).cuda(), torch.from_numpy(ref[None]).cuda())[0])
        want = ref_fn(img, ref)
        assert abs(got - want) <= TOL * abs(want), (name, got, want)
