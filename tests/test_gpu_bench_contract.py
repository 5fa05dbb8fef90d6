"""bench.py's one-line JSON contract on the GPU box: a short run in a child process (with --full the bench spawns its
CPU-baseline processes before it touches HIP, so it has to be its own interpreter), parsed and checked field by field."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '4', '--warmup', '2'] + extra,
                         cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_line_contract():
    line = _run(['--full', '--cpu-seconds', '2'])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in line, k
    assert line['n_gpus'] == 1 and line['steps'] == 4 and line['warmup'] == 2 and line['vs_baseline'] is None
    assert isinstance(line['value'], float) and line['value'] > 0
    assert abs(line['value'] - line['config']['restarts_total'] * 4 / (line['ms_per_step'] * 4e-3)) < 1e-6 * line['value']
    r = line['roofline']
    assert r['bound'] in ('hbm', 'mfma', 'fp64_valu') and r['peak'] > 0 and 0 < r['frac'] < 1
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-12
    hb = r.get('hbm_family', r)
    assert hb['bound'] == 'hbm' and 0 < hb['frac'] < 1 and hb['unit'] == 'GB/s'
    c = line['cpu_baseline']
    assert c['kind'] == 'port' and c['value'] > 0 and c['cores'] >= 1 and c['sample']
    assert 'workload' in line['config'] and 'model' not in line['config']


@pytest.mark.gpu
def test_bench_line_without_profile_brackets():
    line = _run(['--no-cpu-baseline', '--no-roofline'])
    assert line['value'] > 0 and line['roofline'] is None and line['cpu_baseline'] is None


@pytest.mark.gpu
def test_bench_plain_run_dumps_outputs(tmp_path):
    """a plain run times one window of exactly K steps, measures nothing else, and --dump-outputs writes the state the last
    timed step left as float arrays (at most 64 MB)"""
    line = _run(['--dump-outputs', str(tmp_path)])
    assert line['steps'] == 4 and line['value'] > 0 and line['ms_per_step'] > 0
    assert len(line['repeats']['windows_ms']) == 1
    assert abs(line['repeats']['windows_ms'][0] - 4 * line['ms_per_step']) < 1e-9 * line['repeats']['windows_ms'][0]
    assert line['roofline'] is None and line['cpu_baseline'] is None and 'kernel_families_ms' not in line
    files = sorted(os.listdir(tmp_path))
    for name in ('density', 'reciprocal_density', 'support', 'error_last_step', 'best_error'):
        assert name + '.npy' in files, name
    total = 0
    B = line['config']['restarts_per_gpu']
    for f in files:
        v = np.load(os.path.join(tmp_path, f))
        assert v.dtype in (np.float32, np.float64), (f, v.dtype)
        total += v.nbytes
    assert total <= 64 * 2 ** 20
    err = np.load(os.path.join(tmp_path, 'error_last_step.npy'))
    assert err.shape == (B,) and np.all(np.isfinite(err)) and np.all(err > 0)
    rho = np.load(os.path.join(tmp_path, 'density.npy'))
    assert rho.shape[0] == B and rho.shape[-1] == 2 and np.all(np.isfinite(rho)) and np.abs(rho).max() > 0
