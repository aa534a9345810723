"""The tracker's routing from a GPU scorer's output column to `<metric>.txt`, with every scorer replaced by a stand-in (no GPU is
needed: the tracker's GPU paths run on CPU tensors then).  Each column carries its own base, so a crossed column, a scorer that
runs twice or a scorer that runs for a refused name shows in a file or in a call count."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

NAMES = ['mse', 'ssim', 'psnr', 'ms_ssim', 'gmsd', 'piqe', 'lpips', 'lpips-vgg', 'niqe', 'brisque']
BASE = {'mse': 10, 'ssim': 20, 'psnr': 30, 'ms_ssim': 40, 'gmsd': 50, 'piqe': 60, 'lpips': 70, 'lpips-vgg': 80, 'niqe': 90, 'brisque': 100}
BATCHES = (3, 2, 1)
UNUSED = 1e6        # gmsd's second column (the mean GMS): no file may hold it


class _StandIn:
    """A wrapper's call shape (flags, no `ref` for a no-reference metric, `out=` or a returned tensor) with base + arange(n) in
    every column."""

    def __init__(self, *bases, forbidden=False, returns_first=False):
        self.bases, self.forbidden, self.returns_first, self.calls = bases, forbidden, returns_first, []

    def __call__(self, img, ref=None, clip=True, out=None, **flags):
        assert not self.forbidden, 'a scorer ran although its scores were handed in'
        assert clip is True
        self.calls.append(flags)
        n = img.shape[0]
        rows = torch.stack([b + torch.arange(n, dtype=torch.float64) for b in self.bases], dim=1)
        rows = rows[:, 0] if len(self.bases) == 1 else rows
        if out is not None:
            out.copy_(rows)
            rows = out
        return rows[:, 0] if self.returns_first else rows       # (GMSD writes two columns and returns the first)

    def saturation(self):
        return 0


def _tracker(tmp_path, monkeypatch, sub, forbidden=False):
    from evreal_amd import build, eval_metrics as em
    build.build(verbose=False)
    for env in (em.FR_METRICS_ENV, em.PIQE_ENV, em.GMSD_ENV):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setattr(em, '_pyiqa_factory', SimpleNamespace(list_of_metrics=[]))
    T = em.EvalMetricsTracker
    stand = {k: _StandIn(*b, forbidden=forbidden, returns_first=k == 'gmsd') for k, b in dict(
        gpu=(10, 20), fr=(30, 40), gmsd=(50, UNUSED), piqe=(60,), lpips=(70,), lpips_vgg=(80,), niqe=(90,), brisque=(100,)).items()}
    for k in ('lpips', 'lpips_vgg', 'niqe', 'brisque', 'piqe'):
        monkeypatch.setattr(T, f'_{k}_cache', [True, stand[k]])
    t = T(output_dir=str(tmp_path / sub), quan_eval_metric_names=list(NAMES), has_reference_frames=True)
    t._gpu, t._fr, t._gmsd = stand['gpu'], stand['fr'], stand['gmsd']
    return t, stand


def _feed(t, H, W, scores=None):
    k = 0
    for n in BATCHES:
        idx = list(range(k, k + n))
        pre = None if scores is None else {name: v[k:k + n] for name, v in scores.items()}
        t.update_batch(idx, torch.zeros((n, H, W)), torch.zeros((n, H, W)), [0.01 * i for i in idx], None, scores=pre)
        k += n
    t.finalize(k - 1)


def _lines(t, name):
    return open(f'{t.output_dir}/{name}.txt').read().splitlines()


IN_BATCH = [j for n in BATCHES for j in range(n)]       # a frame's position in the batch it arrived in


def test_every_column_reaches_its_own_file(tmp_path, monkeypatch, capsys):
    t, stand = _tracker(tmp_path, monkeypatch, 'out')
    assert [m.name for m in t.metrics] == NAMES and t.wants_precomputed() == NAMES
    _feed(t, 200, 200)
    means = t.get_mean_scores()
    for name in NAMES:
        assert _lines(t, name) == ['{} {:.5f}'.format(i, BASE[name] + j) for i, j in enumerate(IN_BATCH)], name
        assert means[name] == pytest.approx(BASE[name] + np.mean(IN_BATCH), abs=1e-12), name
    for k, s in stand.items():
        assert len(s.calls) == len(BATCHES), k          # one launch set per batch
    assert stand['gpu'].calls[0] == dict(mse=True, ssim=True) and stand['fr'].calls[0] == dict(psnr=True, ms_ssim=True)
    out = capsys.readouterr().out
    assert 'Exception in metric' not in out and 'Unknown metric' not in out


def test_handed_in_scores_are_booked_and_nothing_runs(tmp_path, monkeypatch):
    t, _ = _tracker(tmp_path, monkeypatch, 'pre', forbidden=True)
    scores = {name: 1000.0 * (k + 1) + np.arange(6) for k, name in enumerate(NAMES)}
    _feed(t, 200, 200, scores)
    means = t.get_mean_scores()
    for k, name in enumerate(NAMES):
        assert _lines(t, name) == ['{} {:.5f}'.format(i, 1000.0 * (k + 1) + i) for i in range(6)], name
        assert means[name] == pytest.approx(1000.0 * (k + 1) + 2.5, abs=1e-9), name


def test_refused_names_stay_empty_and_their_neighbours_are_full(tmp_path, monkeypatch, capsys):
    t, stand = _tracker(tmp_path, monkeypatch, 'small')
    _feed(t, 8, 200)
    out = capsys.readouterr().out
    means = t.get_mean_scores()
    for name in NAMES:
        if name in ('ms_ssim', 'lpips-vgg'):
            assert _lines(t, name) == [] and means[name] == -1, name
            assert out.count(f'Exception in metric {name}: ') == 1
        else:
            assert _lines(t, name) == ['{} {:.5f}'.format(i, BASE[name] + j) for i, j in enumerate(IN_BATCH)], name
    assert out.count('Exception in metric') == 2
    assert stand['lpips_vgg'].calls == []               # refused from the shape: never launched
    assert stand['fr'].calls == [dict(psnr=True, ms_ssim=False)] * len(BATCHES)
