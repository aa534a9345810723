"""PIQE on the GPU (evr_piqe_*, evreal_amd/nriqa.py) against the numpy oracle (tests/piqe_ref.py), and the `-qm piqe` path of
the tracker and of evaluate() -- with no model file anywhere -- against the oracle fed through the reference's four-frame
queue.  The input set is piqe_ref.inputs(); tests/test_piqe_cpu.py holds it to coverage of the five block classes and to a
margin >= 1e-6 of every deciding quantity from its threshold, so no block is left out of the flag comparison here."""
import numpy as np
import pytest
import torch

import piqe_ref as P
from test_gpu_nriqa import _compare_lines, _queue_lines, _write_tree

pytestmark = pytest.mark.gpu

MARGIN = 1e-9           # a block whose oracle margin is below this may be left out of the flag comparison ...
MAX_LEFT_OUT = 0        # ... but with this input set none is


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def piqe():
    from evreal_amd.nriqa import PIQE
    return PIQE()


@pytest.fixture(scope='module')
def cases():
    """[(name, clip, frame, oracle blocks)]: computed once, shared, never modified."""
    out = []
    for name, a in P.inputs():
        out.append((name, True, a, P.blocks(a, True)))
        if name in P.UNCLIPPED:
            x = P.unclipped(a)
            out.append((name, False, x, P.blocks(x, False)))
    return out


def test_blocks_match_the_oracle(piqe, cases):
    for name, clip, a, want in cases:
        var, flags = piqe.blocks(_cuda(a[None]), clip=clip)
        var, flags = var[0].cpu().numpy(), flags[0].cpu().numpy()
        assert var.shape == want['var'].shape and flags.shape == want['flags'].shape, name
        err = np.abs(var - want['var'])
        print(f"{name} clip={clip}: {var.size} blocks, max |dvar| {err.max():.3e}, oracle margin {want['margin'].min():.3e}")
        np.testing.assert_allclose(var, want['var'], rtol=1e-10, atol=1e-14, err_msg=f'{name} clip={clip}')
        keep = want['margin'] >= MARGIN
        assert np.count_nonzero(~keep) <= MAX_LEFT_OUT, name
        assert np.array_equal(flags[keep], want['flags'][keep]), (name, clip, np.argwhere(flags != want['flags']))


def test_scores_match_the_oracle(piqe, cases):
    for name, clip, a, want in cases:
        got = float(piqe(_cuda(a[None]), clip=clip)[0])
        ref = P.score_blocks(want)
        print(f'{name} clip={clip}: {got!r} (oracle {ref!r})')
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9, err_msg=f'{name} clip={clip}')
    assert float(piqe(_cuda(np.full((1, 40, 40), 0.4, np.float32)))[0]) == 100.0


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def test_bitwise_independent_of_batch_and_position(piqe):
    rng = np.random.default_rng(7)
    x = dict(P.inputs())['81x113 texture + noise']
    others = np.stack([(P.texture(81, 113, s) + 0.05 * rng.standard_normal((81, 113))).astype(np.float32) for s in range(5)])
    alone = _bits(piqe(_cuda(x[None])))
    var1, fl1 = piqe.blocks(_cuda(x[None]))
    for pos in (0, 2, 4):
        batch = others.copy()
        batch[pos] = x
        assert _bits(piqe(_cuda(batch)))[pos] == alone[0], pos
        var5, fl5 = piqe.blocks(_cuda(batch))
        assert torch.equal(var5[pos].view(torch.int64), var1[0].view(torch.int64)) and torch.equal(fl5[pos], fl1[0]), pos
    full = _bits(piqe(_cuda(others)))
    ones = np.concatenate([_bits(piqe(_cuda(others[i:i + 1]))) for i in range(5)])
    assert np.array_equal(full, ones)


def test_constant_and_nan_frames_leave_their_neighbours_alone(piqe):
    rng = np.random.default_rng(8)
    frames = np.stack([(P.texture(81, 113, s) + 0.05 * rng.standard_normal((81, 113))).astype(np.float32) for s in range(5)])
    clean = _bits(piqe(_cuda(frames), clip=False))
    frames[1] = 0.4
    frames[3, 20:30, 40:60] = np.nan
    got = piqe(_cuda(frames), clip=False)
    assert float(got[1]) == 100.0
    assert np.array_equal(_bits(got)[[0, 2, 4]], clean[[0, 2, 4]])
    var, flags = piqe.blocks(_cuda(frames[3:4]), clip=False)
    bad = torch.isnan(var[0])
    assert bad.any() and not bad.all() and not flags[0][bad].any()          # comparisons with NaN are false: inactive blocks


def test_more_frames_than_one_grid_axis_holds(piqe):
    """Frames ride the grid's y axis, chunked at 65535: 65537 one-block frames against the first and the last 100 computed
    alone."""
    n = 65537
    x = torch.rand((n, 16, 16), generator=torch.Generator(device='cuda').manual_seed(65537), device='cuda')
    full = piqe(x)
    var, flags = piqe.blocks(x)
    assert bool(torch.isfinite(full).all())
    for sl in (slice(0, 100), slice(n - 100, n)):
        assert torch.equal(piqe(x[sl].contiguous()).view(torch.int64), full[sl].view(torch.int64))
        v, f = piqe.blocks(x[sl].contiguous())
        assert torch.equal(v.view(torch.int64), var[sl].view(torch.int64)) and torch.equal(f, flags[sl])


def test_workspace_and_argument_refusals(piqe):
    from evreal_amd import lib as L
    lib = L.load()
    x = _cuda(np.stack([dict(P.inputs())['17x33']] * 3))
    out = torch.full((3,), -7.0, dtype=torch.float64, device='cuda')
    var = torch.full((3, 2, 3), -7.0, dtype=torch.float64, device='cuda')
    flags = torch.full((3, 2, 3), 77, dtype=torch.uint8, device='cuda')
    need = int(lib.evr_piqe_workspace_bytes(3, 17, 33))
    assert need > 0 and lib.evr_piqe_workspace_bytes(0, 17, 33) == 0 and lib.evr_piqe_workspace_bytes(3, 0, 33) == 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    st = L.stream_ptr()

    def refused(rc, code):
        assert rc == code and lib.evr_last_error().decode().startswith('evr_piqe_'), (rc, lib.evr_last_error())

    refused(lib.evr_piqe_score(L.ptr(x), 3, 17, 33, 1, L.ptr(out), L.ptr(ws), need - 1, st), -3)
    refused(lib.evr_piqe_score(L.ptr(x), 3, 17, 33, 1, L.ptr(out), None, need, st), -3)
    refused(lib.evr_piqe_score(None, 3, 17, 33, 1, L.ptr(out), L.ptr(ws), need, st), -1)
    refused(lib.evr_piqe_score(L.ptr(x), 3, 17, 33, 1, None, L.ptr(ws), need, st), -1)
    refused(lib.evr_piqe_score(L.ptr(x), 0, 17, 33, 1, L.ptr(out), L.ptr(ws), need, st), -1)
    refused(lib.evr_piqe_score(L.ptr(x), -1, 17, 33, 1, L.ptr(out), L.ptr(ws), need, st), -1)
    refused(lib.evr_piqe_score(L.ptr(x), 3, 0, 33, 1, L.ptr(out), L.ptr(ws), need, st), -1)
    refused(lib.evr_piqe_blocks(L.ptr(x), 3, 17, 33, 1, None, L.ptr(flags), L.ptr(ws), need, st), -1)
    refused(lib.evr_piqe_blocks(L.ptr(x), 3, 17, 33, 1, L.ptr(var), None, L.ptr(ws), need, st), -1)
    refused(lib.evr_piqe_blocks(L.ptr(x), 0, 17, 33, 1, L.ptr(var), L.ptr(flags), L.ptr(ws), need, st), -1)
    refused(lib.evr_piqe_blocks(L.ptr(x), 3, 17, 33, 1, L.ptr(var), L.ptr(flags), L.ptr(ws), need - 1, st), -3)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((var == -7.0).all()) and bool((flags == 77).all())      # nothing was launched
    assert lib.evr_piqe_score(L.ptr(x), 3, 17, 33, 1, L.ptr(out), L.ptr(ws), need, st) == 0
    torch.cuda.synchronize()
    assert np.all(np.isfinite(out.cpu().numpy())) and bool((out != -7.0).all())


def test_tracker_books_piqe_like_the_reference_queue(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em
    monkeypatch.chdir(tmp_path)                      # no model file anywhere
    monkeypatch.delenv(em.PIQE_ENV, raising=False)
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['piqe'], has_reference_frames=False)
    assert [m.name for m in t.metrics] == ['piqe'] and t.wants_precomputed() == ['piqe']
    rng = np.random.default_rng(9)
    frames = [(P.texture(81, 113, s) + 0.02 * (s + 1) * rng.standard_normal((81, 113))).astype(np.float32) for s in range(6)]
    idx, k = list(range(6)), 0
    for n in (1, 3, 2):                              # one full group of four, and a tail of two at finalize
        t.update_batch(idx[k:k + n], _cuda(np.stack(frames[k:k + n])), None, [0.01 * i for i in idx[k:k + n]], None)
        k += n
    assert len(open(tmp_path / 'out' / 'piqe.txt').read().splitlines()) == 4
    t.finalize(idx[-1])
    want = _queue_lines(idx, [P.piqe(f) for f in frames])
    got = open(tmp_path / 'out' / 'piqe.txt').read()
    assert len(got.splitlines()) == 6
    _compare_lines(got, want)
    assert t.get_mean_scores()['piqe'] == pytest.approx(np.mean([P.piqe(f) for f in frames]), rel=1e-9)


def test_tracker_computes_piqe_on_the_processed_frames_under_hist_eq(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em
    from evreal_amd.prepost import histogram_equalization
    monkeypatch.chdir(tmp_path)
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['piqe'], has_reference_frames=False,
                              hist_eq='global')
    assert t.wants_precomputed() == []
    rng = np.random.default_rng(10)
    frames = np.stack([(0.3 + 0.3 * P.texture(81, 113, s) + 0.03 * rng.standard_normal((81, 113))).astype(np.float32) for s in range(4)])
    t.update_batch([0, 1, 2, 3], _cuda(frames), None, [0.0, 0.1, 0.2, 0.3], None)
    t.finalize(3)
    eq = histogram_equalization(torch.clamp(_cuda(frames), 0.0, 1.0).contiguous(), 'global').cpu().numpy()
    _compare_lines(open(tmp_path / 'out' / 'piqe.txt').read(), _queue_lines([0, 1, 2, 3], [P.piqe(f) for f in eq]))


@pytest.fixture(scope='module')
def evaluated(tmp_path_factory):
    """evaluate() with -qm piqe on a tiny sequence tree without frames and without any model file, once with batch_sequences 1
    and once with 2 (the same two sequences) -> {batch_sequences: (root, sequence names, printed text, results)}."""
    import contextlib
    import io
    import os
    from evreal_amd import eval as ev
    out, cwd = {}, os.getcwd()
    old = {k: os.environ.get(k) for k in ('EVREAL_BATCH_SEQUENCES', 'EVREAL_GPU_PIQE')}
    os.environ.pop('EVREAL_GPU_PIQE', None)
    try:
        for bs in (1, 2):
            root = tmp_path_factory.mktemp('piqe_eval%d' % bs)
            names = _write_tree(str(root), False, (81, 82))
            os.environ['EVREAL_BATCH_SEQUENCES'] = str(bs)
            os.chdir(root)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                res = ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['piqe'])
            out[bs] = (root, names, buf.getvalue(), res)
    finally:
        os.chdir(cwd)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def _out(root, name):
    return root / 'outputs' / 'k3k' / 'NR' / name / 'FireNet'


@pytest.mark.parametrize('batch_sequences', [1, 2])
def test_evaluate_without_frames_or_model_files_writes_piqe(evaluated, batch_sequences):
    from PIL import Image
    root, names, text, res = evaluated[batch_sequences]
    assert 'Unknown metric' not in text and 'Exception' not in text, text
    total = 0
    for name in names:
        o = _out(root, name)
        idx = [int(l.split()[0]) for l in open(o / 'timestamps.txt').read().splitlines()]
        got = open(o / 'piqe.txt').read()
        assert len(idx) >= 8 and len(got.splitlines()) == len(idx)      # one line per frame
        scores = [P.piqe(np.asarray(Image.open(o / 'frame_{:010d}.png'.format(i)), dtype=np.float32) / np.float32(255.0))
                  for i in idx]
        _compare_lines(got, _queue_lines(idx, scores))
        total += len(idx)
    dm = res['k3k'][0][0]                                               # the dataset's row of the printed table
    assert dm.get_count('piqe') == total
    assert dm.get_average('piqe') != -1 and 0.0 < dm.get_average('piqe') <= 100.0
    assert 'PIQE' in text


def test_evaluate_files_do_not_depend_on_batch_sequences(evaluated):
    (r1, names, _, _), (r2, _, _, _) = evaluated[1], evaluated[2]
    for name in names:
        for f in ('piqe.txt', 'timestamps.txt'):
            a, b = open(_out(r1, name) / f).read(), open(_out(r2, name) / f).read()
            assert a == b and a, (name, f)


def test_piqe_next_to_mse_leaves_mse_unchanged(tmp_path, monkeypatch):
    from evreal_amd import eval as ev
    monkeypatch.setenv('EVREAL_BATCH_SEQUENCES', '2')
    monkeypatch.delenv('EVREAL_GPU_PIQE', raising=False)
    names = _write_tree(str(tmp_path), True, (91, 92))
    monkeypatch.chdir(tmp_path)
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse'])
    before = {n: open(_out(tmp_path, n) / 'mse.txt').read() for n in names}
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'piqe'])
    for n in names:
        assert open(_out(tmp_path, n) / 'mse.txt').read() == before[n] and before[n]
        assert len(open(_out(tmp_path, n) / 'piqe.txt').read().splitlines()) == len(before[n].splitlines())
