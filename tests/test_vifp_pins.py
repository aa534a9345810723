"""VIFp pinned to sewar (`sewar.vifp`: the pixel-domain multi-scale form of the LIVE release, in fp64) where sewar exists: the
oracle (CPU) and the kernel (`-m gpu`) against sewar.vifp on the 255 * frame float arrays.  It is the same algorithm through
another filter routine, so 1e-9 relative.  The module skips where sewar is missing -- nothing is installed for it -- and until it
has run the parity with an outside package is unpinned.  A convention it contradicts (the taps, the valid region, the even
indices of the decimation, EPS = 1e-10, the order of the threshold rules) is fixed in tests/vifp_ref.py and csrc/vifp.hip
together."""
import numpy as np
import pytest

import vifp_ref as V
from thirdparty_refs import image_pairs

sewar = pytest.importorskip('sewar')

TOL = 1e-9      # relative


def _pairs():
    return [p for p in image_pairs() if p[0] != 'constant']


def _sewar(img, ref):
    """sewar.vifp(GT, P): the reference first."""
    return float(sewar.vifp(255.0 * ref.astype(np.float64), 255.0 * img.astype(np.float64)))


def test_oracle_matches_sewar():
    for name, img, ref in _pairs():
        got, want = V.vifp(img, ref), _sewar(img, ref)
        assert abs(got - want) <= TOL * abs(want), (name, got, want)


@pytest.mark.gpu
def test_kernel_matches_sewar():
    import torch
    from evreal_amd.prepost import VIFP
    vf = VIFP()
    for name, img, ref in _pairs():
        got = float(vf(torch.from_numpy(img[None]).cuda(), torch.from_numpy(ref[None]).cuda())[0])
        want = _sewar(img, ref)
        assert abs(got - want) <= TOL * abs(want), (name, got, want)
