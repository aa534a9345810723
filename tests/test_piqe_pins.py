"""PIQE pinned to pyiqa (the reference's `-qm piqe`, utils/eval_metrics.py:110-147) where pyiqa exists: the oracle (CPU) and
the kernels (`-m gpu`) against pyiqa.create_metric('piqe') called as the reference calls it (a gray frame replicated to
three channels, eval_utils.py:46-54).  PIQE has no weights, so pyiqa alone is enough; the two comparisons skip where it is
missing.  A convention they contradict (the centre columns, the 'post' padding, the input rounding) is fixed in
tests/piqe_ref.py and csrc/nriqa.hip together.  The last test runs the same helpers against the oracle, so the plumbing is
exercised where pyiqa is absent."""
import numpy as np
import pytest

import piqe_ref as P

TOL = 1e-4      # relative to max(|score|, 1): pyiqa computes in fp32 tensors


def _frames():
    rng = np.random.default_rng(2)
    out = []
    for k, (H, W) in enumerate(((260, 346), (81, 113), (96, 128))):
        a = P.texture(H, W, k) + 0.03 * (k + 1) * rng.standard_normal((H, W))
        out.append(np.clip(P.block_average(a) if k == 2 else a, 0, 1).astype(np.float32))
    return out


def _pyiqa_metric():
    pyiqa = pytest.importorskip('pyiqa')
    import torch
    metric = pyiqa.create_metric('piqe', device='cpu')
    return lambda v: float(metric(torch.from_numpy(v)[None].repeat(3, 1, 1)[None]).squeeze())


def _close(got, want):
    return abs(got - want) <= TOL * max(abs(want), 1.0)


def _kernel_scores(frames):
    import torch
    from evreal_amd.nriqa import PIQE
    piqe = PIQE()
    return [float(piqe(torch.from_numpy(v[None]).cuda())[0]) for v in frames]


def test_oracle_matches_pyiqa():
    ref = _pyiqa_metric()
    for v in _frames():
        got, want = P.piqe(v), ref(v)
        assert _close(got, want), (v.shape, got, want)


@pytest.mark.gpu
def test_kernel_matches_pyiqa():
    ref = _pyiqa_metric()
    frames = _frames()
    for v, got in zip(frames, _kernel_scores(frames)):
        want = ref(v)
        assert _close(got, want), (v.shape, got, want)


@pytest.mark.gpu
def test_pin_helpers_run_against_the_oracle():
    frames = _frames()
    scores = [P.piqe(v) for v in frames]
    assert np.std(scores) > 1.0                     # the frames are told apart
    for v, got, want in zip(frames, _kernel_scores(frames), scores):
        assert _close(got, want), (v.shape, got, want)
