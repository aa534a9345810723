"""The record that tests/test_gpu_etnet_tokens.py can fail: at each of its cases, four kernel bugs restated in the float64 oracle move
every tensor they touch by at least ten times that test's limit (computed from e_32 and T_64 alone).  No GPU, no reference tree.

The bugs, one at a time, through hooks on oracle.model's helpers kept here:
    last_q    the last query misses the last key in every attention (a tail mask off by one)
    all_q     every query misses the last key
    pos_row   the position row of sequence 1 is taken from the global row n L + l instead of l (moves sequence 1 only)
    ln_255    LayerNorm divides the squared deviations by 255 instead of 256
Attention and LayerNorm sit behind the encoders' input, so words0..2 and the ConvLSTM states stay; everything else must move.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model as omod
import test_gpu_etnet_tokens as g

MARGIN = 10.0
AFTER_ATTENTION = [k for k in g.TOKENS if not k.startswith('words')] + g.IMAGES


def _mha_missing_last_key(all_queries):
    def mha(sd, p, q_in, k_in, v_in, nhead=8):
        E = q_in.shape[-1]
        W, b = sd[p + '.in_proj_weight'], sd[p + '.in_proj_bias']
        q = F.linear(q_in, W[:E], b[:E]); k = F.linear(k_in, W[E:2 * E], b[E:2 * E]); v = F.linear(v_in, W[2 * E:], b[2 * E:])
        L, N, _ = q.shape; S = k.shape[0]; d = E // nhead
        q = q.reshape(L, N * nhead, d).transpose(0, 1); k = k.reshape(S, N * nhead, d).transpose(0, 1)
        v = v.reshape(S, N * nhead, d).transpose(0, 1)
        logits = torch.bmm(q, k.transpose(1, 2)) / (d ** 0.5)
        logits[:, (slice(None) if all_queries else L - 1), S - 1] = float('-inf')
        o = torch.bmm(torch.softmax(logits, dim=-1), v).transpose(0, 1).reshape(L, N, E)
        return F.linear(o, sd[p + '.out_proj.weight'], sd[p + '.out_proj.bias'])
    return mha


def _add_pos_global_row(words, table):
    n, L, _ = words.shape
    wide = omod.sine_position_table(n * L).to(words.dtype)
    return words + wide.reshape(n, L, -1)


def _layer_norm_div(div):
    def layer_norm(sd, p, x):
        d = x - x.mean(-1, keepdim=True)
        return d / torch.sqrt((d * d).sum(-1, keepdim=True) / div + 1e-5) * sd[p + '.weight'] + sd[p + '.bias']
    return layer_norm


MUTATIONS = {'last_q': ('_mha', _mha_missing_last_key(False)), 'all_q': ('_mha', _mha_missing_last_key(True)),
             'pos_row': ('_add_pos', _add_pos_global_row), 'ln_255': ('_layer_norm', _layer_norm_div(255))}


def test_the_hooks_restate_the_oracle(monkeypatch):
    """Each hook with its bug taken out is the oracle's own helper: what a mutation moves is the bug and nothing else."""
    x = torch.randn(5, 2, 256, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 3 + 1
    sd = {'n.weight': torch.rand(256, dtype=torch.float64), 'n.bias': torch.rand(256, dtype=torch.float64)}
    assert float((_layer_norm_div(256)(sd, 'n', x) - omod._layer_norm(sd, 'n', x)).abs().max()) < 1e-12

    def mha_extra_key(sd, p, q_in, k_in, v_in, nhead=8):      # one more key, which every query then misses
        return _mha_missing_last_key(True)(sd, p, q_in, torch.cat((k_in, k_in[-1:] + 1)), torch.cat((v_in, v_in[-1:] + 1)))
    t64, _ = g.references(0)
    monkeypatch.setattr(omod, '_mha', mha_extra_key)
    got = g.oracle_run(0, torch.float64)
    for k in g.TOKENS + g.IMAGES:
        assert float(np.abs(got[k] - t64[k]).max()) < 1e-11, k


@pytest.mark.parametrize('ci', range(len(g.CASES)), ids=g.IDS)
@pytest.mark.parametrize('mut', list(MUTATIONS))
def test_restated_kernel_bugs_exceed_the_gpu_limit(monkeypatch, mut, ci):
    t64, t32 = g.references(ci)
    name, fn = MUTATIONS[mut]
    monkeypatch.setattr(omod, name, fn)
    got = g.oracle_run(ci, torch.float64)
    monkeypatch.undo()
    affected = (['words0', 'words1', 'words2'] if mut == 'pos_row' else []) + AFTER_ATTENTION
    report, weak = [], []
    for k in g.TOKENS + g.STATES + g.IMAGES:
        sl = slice(1, 2) if mut == 'pos_row' else slice(None)
        moved = float(np.abs(got[k][sl] - t64[k][sl]).max())
        e32 = float(np.abs(t32[k] - t64[k]).max())
        lim = g.limit(k, e32, t64[k])
        report.append(f'  {k:9s} moved {moved:.3e}  e_32 {e32:.3e}  limit {lim:.3e}  x{moved / lim:9.1f}')
        if k in affected:
            if moved < MARGIN * lim:
                weak.append(k)
        else:
            assert moved == 0.0, (k, moved)          # upstream of the bug
        if mut == 'pos_row':                          # sequence 0 reads its own rows either way
            assert np.array_equal(got[k][:1], t64[k][:1]), k
    print(f'\n[{mut} {g.IDS[ci]}]\n' + '\n'.join(report))
    assert not weak, (weak, '\n'.join(report))
