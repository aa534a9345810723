"""N>1 path on CPU: world-size-2 gloo process group reproduces MetricTracker's weighted average
(eval.py:259-266) from per-rank partial sums, and the sequence assignment is a deterministic partition."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from evreal_amd.dist import assign_sequences, reduce_metric_sums
from oracle.metrics import MetricTracker
from conftest import GOLDEN


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


SEQS = [  # (name, n_evaluated, {metric: mean score}) -- includes an un-evaluated sequence and a -1 mean
    ('a', 10, {'mse': 0.05, 'ssim': 0.61}), ('b', 30, {'mse': 0.10, 'ssim': 0.40}),
    ('c', 0, {'mse': -1, 'ssim': -1}), ('d', 7, {'mse': 0.31, 'ssim': 0.12}), ('e', 19, {'mse': 0.02, 'ssim': 0.88}),
]
COSTS = [5.0, 9.0, 1.0, 3.0, 7.0]


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    mine = assign_sequences(COSTS, world)[rank]
    sums = torch.zeros((1, 3), dtype=torch.float64)
    for i in mine:
        _, n, sc = SEQS[i]
        if n == 0:
            continue                               # eval.py:260-261
        sums[0, 0] += sc['mse'] * n; sums[0, 1] += sc['ssim'] * n; sums[0, 2] += n
    tot = reduce_metric_sums(sums, dist)
    q.put((rank, mine, tot.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_matches_metric_tracker():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs: p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60); assert p.exitcode == 0
    mt = MetricTracker()
    for _, n, sc in SEQS:
        for k, v in sc.items():
            mt.update(k, v, n)
    seen = sorted(i for _, mine, _ in res for i in mine)
    assert seen == list(range(len(SEQS)))          # a partition: every sequence on exactly one rank
    for _, _, tot in res:                           # every rank holds the global totals
        t = np.array(tot)
        assert int(t[0, 2]) == mt.count('mse') == 66
        assert abs(t[0, 0] / t[0, 2] - mt.average('mse')) < 1e-15
        assert abs(t[0, 1] / t[0, 2] - mt.average('ssim')) < 1e-15


def test_assign_sequences_lpt():
    plan = assign_sequences([5, 9, 1, 3, 7], 2)
    assert sorted(sum(plan, [])) == [0, 1, 2, 3, 4]
    loads = [sum([5, 9, 1, 3, 7][i] for i in p) for p in plan]
    assert abs(loads[0] - loads[1]) <= 3
    assert assign_sequences([5, 9, 1, 3, 7], 2) == plan             # deterministic
    assert assign_sequences([1.0] * 3, 8)[3:] == [[]] * 5           # more ranks than sequences
    assert reduce_metric_sums(torch.ones((1, 3), dtype=torch.float64)).tolist() == [[1.0, 1.0, 1.0]]


def _fold_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from evreal_amd.eval import fold_dataset_metrics
    from evreal_amd.eval_metrics import MetricTracker as MT
    dm = MT()
    if rank == 0:       # rank 1 owns no sequence of this dataset: its tracker stays empty
        dm.update('mse', 0.05, 10); dm.update('ssim', 0.61, 10); dm.update('lpips', 0.33, 10)
        dm.update('mse', 0.10, 30); dm.update('ssim', 0.40, 30); dm.update('lpips', 0.20, 30)
    out = fold_dataset_metrics(dm, ['mse', 'ssim', 'LPIPS', 'niqe'], dist)      # (a mixed-case -qm name: trackers key it lower-cased)
    q.put((rank, {k: (v['total'], v['count'], v['average']) for k, v in out.data_dict.items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_fold_keeps_every_tracked_metric():
    """The multi-rank table must carry the same columns as the single-rank one (lpips and plug-in metrics included);
    a requested metric nobody scored stays absent."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_fold_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs: p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60); assert p.exitcode == 0
    for _, d in res:
        assert list(d) == ['mse', 'ssim', 'lpips']
        assert d['lpips'][1] == 40 and abs(d['lpips'][2] - (0.33 * 10 + 0.20 * 30) / 40) < 1e-15
        assert abs(d['mse'][2] - 0.0875) < 1e-15


def test_checkpoint_config_parser_shim(tmp_path):
    """E2VID+/FireNet+/HyperE2VID checkpoints pickle a parse_config.ConfigParser (reference parse_config.py:1-22) whose
    only attribute is `_config`; eval.py:150-151 reads config['arch']."""
    import sys, types
    from evreal_amd.eval import _load_checkpoint
    mod = types.ModuleType('parse_config')

    class ConfigParser:
        def __init__(self, config):
            self._config = config
    ConfigParser.__module__ = 'parse_config'
    ConfigParser.__qualname__ = 'ConfigParser'
    mod.ConfigParser = ConfigParser
    sys.modules['parse_config'] = mod
    try:
        torch.save({'config': ConfigParser({'arch': {'type': 'FireNet', 'args': {'num_bins': 5}}}),
                    'state_dict': {}}, tmp_path / 'm.pth')
    finally:
        del sys.modules['parse_config']
    ck = _load_checkpoint(str(tmp_path / 'm.pth'))
    assert ck['config']['arch']['type'] == 'FireNet' and ck['config']['arch']['args'] == {'num_bins': 5}
    assert ck['config'].config['arch']['type'] == 'FireNet'
    # the shipped FireNet+ checkpoint's own pickle (legacy torch format), its tensors dropped (tests/golden/make_golden.py)
    ck = _load_checkpoint(os.path.join(GOLDEN, 'firenetplus_ckpt_layout.pth'))
    assert ck['config']['arch']['type'] == 'FireNet' and 'num_bins' in ck['config']['arch']['args']


def _cost_worker(rank, world, port, root, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from evreal_amd import eval as ev
    if rank == 1:       # a rank-local read failure (NFS hiccup, permissions): this rank could not have computed the costs itself
        def boom(*a, **k):
            raise OSError("simulated rank-local failure")
        ev.MemMapDataset = boom
    vm = {'method': 'k_events', 'k': 500, 'sliding_window_w': 0}
    seqs = [{'name': n, 'sequence_path': os.path.join(root, n), 'dataset_kwargs': {'num_bins': 5, 'voxel_method': vm}} for n in ('a', 'b', 'c')]
    costs = ev.sequence_costs(seqs)
    q.put((rank, costs, assign_sequences(costs, world)))
    dist.barrier()
    dist.destroy_process_group()


def test_sequence_costs_come_from_rank_0(tmp_path):
    """every rank must partition the sequences by the SAME cost vector; it is computed on rank 0 and broadcast, so a
    rank that cannot read the files still derives the same plan (and fails later, loudly, on the sequences it owns)."""
    from evreal_amd import synth
    for n, ev_count in (('a', 5000), ('b', 20000), ('c', 9000)):
        synth.write_sequence(str(tmp_path / n), 7, ev_count, 1.0e5, 32, 24, 100.0)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cost_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs: p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60); assert p.exitcode == 0
    assert res[0][1] == res[1][1] == [10 * 32 * 32, 40 * 32 * 32, 18 * 32 * 32]      # windows x padded pixels, from rank 0's files
    assert res[0][2] == res[1][2] and sorted(sum(res[0][2], [])) == [0, 1, 2]


def _load_fail_worker(rank, world, port, root, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from evreal_amd import eval as ev
    os.chdir(root)

    class _Model:      # stands in for a loaded network: the test never reaches a frame loop
        pass

    def loader(model_name, path):
        if rank == 1:
            raise OSError("simulated rank-local checkpoint failure")
        return _Model()
    ev.get_model_from_checkpoint_path = loader
    reached = []
    ev.sequence_costs = lambda seqs: reached.append('collective') or [1] * len(seqs)      # the first collective of the dataset loop
    out = ev.eval_method_with_config({'name': 'std'}, 'M', [{'name': 'D', 'sequences': [{'name': 's'}]}], ['mse'])
    q.put((rank, out, reached))
    dist.barrier()
    dist.destroy_process_group()


def test_ranks_agree_on_checkpoint_load_before_the_dataset_collectives(tmp_path):
    """a rank whose checkpoint load fails locally must not leave the others waiting in the dataset loop's collectives
    (sequence_costs' broadcast, the per-dataset all-reduce): the ranks agree on the load first and skip the method everywhere,
    as the reference skips it on its single rank (eval.py:348-352)."""
    import json
    os.makedirs(tmp_path / 'config' / 'method')
    json.dump({"model_name": "E2VID", "model_path": "nowhere.pth"}, open(tmp_path / 'config' / 'method' / 'M.json', 'w'))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_load_fail_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs: p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60); assert p.exitcode == 0
    assert res[0][1] == [] and res[1][1] == []                 # the method is skipped on BOTH ranks ...
    assert res[0][2] == [] and res[1][2] == []                 # ... and neither entered the dataset loop
