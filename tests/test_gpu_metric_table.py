"""evaluate()'s chunk loop with every GPU scorer active at once: all ten names are computed per chunk and handed to the trackers,
and every file equals what a tracker computes by itself from the same frames."""
import json

import numpy as np
import pytest
import torch

from test_gpu_brisque import KEYS, _model as _brisque_model
from test_gpu_nriqa import _compare_lines, _model as _niqe_model, _write_tree

pytestmark = pytest.mark.gpu

NAMES = ['mse', 'ssim', 'psnr', 'ms_ssim', 'gmsd', 'piqe', 'lpips', 'lpips-vgg', 'niqe', 'brisque']


@pytest.fixture()
def model_files(tmp_path, monkeypatch):
    """The synthetic models of the per-metric tests, where the tracker looks for them; every handle is loaded anew."""
    from evreal_amd import eval_metrics as em, weights
    from evreal_amd.nriqa import save_brisque_model, save_niqe_model
    nq, bq = _niqe_model(), _brisque_model()
    paths = {env: str(tmp_path / f) for env, f in ((em.NIQE_MODEL_ENV, 'niqe_model.npz'), (em.BRISQUE_MODEL_ENV, 'brisque_model.npz'),
                                                   (em.LPIPS_WEIGHTS_ENV, 'lpips_alex.pth'), (em.LPIPS_VGG_WEIGHTS_ENV, 'lpips_vgg.pth'))}
    save_niqe_model(paths[em.NIQE_MODEL_ENV], nq['mu'], nq['cov'], 'test')
    save_brisque_model(paths[em.BRISQUE_MODEL_ENV], *(bq[k] for k in KEYS), 'test')
    as_tensors = lambda sd: {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    torch.save(as_tensors(weights.synth_lpips_state_dict(seed=3)), paths[em.LPIPS_WEIGHTS_ENV])
    torch.save(as_tensors(weights.synth_lpips_vgg_state_dict(seed=3)), paths[em.LPIPS_VGG_WEIGHTS_ENV])
    for env, path in paths.items():
        monkeypatch.setenv(env, path)
    for env in (em.FR_METRICS_ENV, em.PIQE_ENV, em.GMSD_ENV):
        monkeypatch.delenv(env, raising=False)
    for cache in ('_lpips_cache', '_lpips_vgg_cache', '_niqe_cache', '_brisque_cache'):
        monkeypatch.setattr(em.EvalMetricsTracker, cache, [False, None])


def test_evaluate_computes_all_ten_names_per_chunk(tmp_path, monkeypatch, model_files):
    from evreal_amd import eval as ev
    from evreal_amd.eval_metrics import EvalMetricsTracker
    names = _write_tree(str(tmp_path), True, (91, 92))
    monkeypatch.chdir(tmp_path)
    cfg_path = tmp_path / 'config' / 'eval' / 'k3k.json'        # (every window is scored: the queues release full groups and a tail)
    cfg_path.write_text(json.dumps(dict(json.loads(cfg_path.read_text()), ts_tol_ms=1e6)))
    out = lambda n: tmp_path / 'outputs' / 'k3k' / 'NR' / n / 'FireNet'
    read = lambda n, files: {f: open(out(n) / (f + '.txt'), 'rb').read() for f in files}
    monkeypatch.setenv('EVREAL_BATCH_SEQUENCES', '2')
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'ssim'])
    plain = {n: read(n, ('mse', 'ssim')) for n in names}

    seen, precomputed = {}, []
    real = EvalMetricsTracker.update_batch

    def spy(self, indices, imgs, refs, img_ts, ref_ts, scores=None, u8=None):
        rec = seen.setdefault(self.output_dir, [])
        rec += [(i, a, b, ts) for i, a, b, ts in zip(indices, imgs.detach().cpu().numpy().copy(), refs.detach().cpu().numpy().copy(), img_ts)]
        precomputed.append(scores is not None and sorted(scores) == sorted(NAMES))
        return real(self, indices, imgs, refs, img_ts, ref_ts, scores=scores, u8=u8)

    monkeypatch.setattr(EvalMetricsTracker, 'update_batch', spy)
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], list(NAMES))
    monkeypatch.setattr(EvalMetricsTracker, 'update_batch', real)
    assert precomputed and all(precomputed)
    cuda = lambda rows, k: torch.from_numpy(np.stack([r[k] for r in rows])).cuda()
    for n in names:
        got = read(n, NAMES)
        assert got['mse'] == plain[n]['mse'] and got['ssim'] == plain[n]['ssim'] and plain[n]['mse']
        evaluated = [int(l.split()[0]) for l in got['mse'].decode().splitlines()]
        assert len(evaluated) >= 8
        rec = [r for r in [v for k, v in seen.items() if k.replace('\\', '/').endswith(f'/{n}/FireNet')][0] if r[0] in set(evaluated)]
        assert [r[0] for r in rec] == evaluated
        # the tracker-only path on the same frames
        t = EvalMetricsTracker(output_dir=str(tmp_path / 'again' / n), quan_eval_metric_names=list(NAMES), has_reference_frames=True)
        assert [m.name for m in t.metrics] == NAMES
        for k in range(0, len(rec), 4):
            part = rec[k:k + 4]
            t.update_batch([r[0] for r in part], cuda(part, 1), cuda(part, 2), [r[3] for r in part], None)
        t.finalize(rec[-1][0])
        for name in NAMES:
            lines = got[name].decode()
            assert [int(l.split()[0]) for l in lines.splitlines()] == evaluated, name
            _compare_lines(lines, open(tmp_path / 'again' / n / (name + '.txt')).read())
