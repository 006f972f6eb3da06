"""`bench.py --dump-outputs DIR`: two runs with the same arguments write the same outputs of their last timed step, bit for
bit; the loss file is the line's `final_loss`, the logits are [B, U, V] and the parameters are every logical element; the
line counts the steps it was asked to time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = 'cfg1'          # the smallest BASELINE.json configuration bench.py times


def _run(out_dir, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '2',
                        '--config', CFG, '--dump-outputs', str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_two_runs_dump_identical_outputs_of_the_last_timed_step(tmp_path):
    from phones_las_amd import model_helper as mh
    c = bench.CONFIGS[CFG]
    lines = [_run(tmp_path / d, 7) for d in ('a', 'b')]
    for line in lines:
        assert line['steps'] == 7 and line['ms_per_step'] > 0 and 'roofline' not in line and 'cpu_baseline' not in line
        assert abs(line['value'] - c['B'] * 1e3 / line['ms_per_step']) < 1e-2 * line['value']
    names = sorted(os.listdir(str(tmp_path / 'a')))
    assert names == ['logits.npy', 'loss.npy', 'params.npy'] and sorted(os.listdir(str(tmp_path / 'b'))) == names
    for n in names:
        a, b = np.load(str(tmp_path / 'a' / n)), np.load(str(tmp_path / 'b' / n))
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), n
    loss = np.load(str(tmp_path / 'a' / 'loss.npy'))
    assert loss.shape == (1,) and round(float(loss[0]), 4) == lines[0]['config']['final_loss']
    assert np.load(str(tmp_path / 'a' / 'logits.npy')).shape == (c['B'], c['U'], c['V'])
    n_params = sum(int(np.prod(shape)) for _, shape, _ in mh.param_table(bench.build_params(c)))
    assert np.load(str(tmp_path / 'a' / 'params.npy')).shape == (n_params,)
