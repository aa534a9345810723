"""The tile map of the skewed 256 x 256 ConvLSTM gate kernel without a GPU: csrc/conv_route.cpp's wide16_tile_map / conv_plan_wide16_map
are pure host code, so tests/wide16_map_cpu.cpp -- a program with its own main() -- is compiled against conv_route.cpp alone with
build.py's hipcc and run.  The program walks every map as the kernel does and checks, for the three headline launches (64 sequences of
346 x 260 on 256 CUs), for a sweep of small and degenerate M / N tiles / CU counts under the rule, and for the forced modes
(EVR_WIDE16_SHORT=all, last=<k>): every pixel in exactly one tile, ranges and tiles end to end, equal tile counts per XCD range, short
tiles last in each range, only the globally last tile past M, EVR_WIDE16_SHORT=0 / an explicit EVR_WIDE_MIN / the other kernels
reproducing the uniform map.  This file pins the headline's totals: full + short tiles 5568 + 320, 1200 + 336 and 300 + 84."""
import json
import os
import subprocess

import pytest

from evreal_amd import build as evr_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'evreal_amd', 'csrc')

pytestmark = pytest.mark.skipif(not os.path.exists(evr_build.HIPCC), reason='no hipcc')


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('wide16_map') / 'wide16_map_cpu')
    cmd = [evr_build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '-Wall', '-Werror',
           '-x', 'hip', os.path.join(ROOT, 'tests', 'wide16_map_cpu.cpp'), os.path.join(CSRC, 'conv_route.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith('EVR_')}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return {d['id']: d for d in map(json.loads, r.stdout.splitlines())}


def test_the_headline_launches_get_the_totals_of_the_rule(rows):
    got = {k: (v['M'], v['nt'], v['full'], v['short']) for k, v in rows.items()}
    assert got == {'enc0.rec': (1486848, 1, 5568, 320), 'enc1.rec': (371712, 2, 1200, 336), 'enc2.rec': (92928, 4, 300, 84)}


def test_the_mixed_grid_is_whole_rounds_and_the_switch_restores_the_uniform_one(rows):
    assert [(rows[k]['grid'], rows[k]['grid_uniform']) for k in ('enc0.rec', 'enc1.rec', 'enc2.rec')] == [(23 * 256, 5808), (12 * 256, 2904), (6 * 256, 1452)]


def test_the_predicted_makespan_beats_whole_rounds(rows):
    for k, rounds in (('enc0.rec', 23), ('enc1.rec', 12), ('enc2.rec', 6)):
        print(f"  {k}: {rows[k]['makespan']} against {rows[k]['makespan_uniform']} full-tile times")
        assert rows[k]['makespan_uniform'] == rounds and rounds - 1 < rows[k]['makespan'] < rounds
