"""bench.py's plain run on the GPU: it times exactly --steps steps, prints the
headline line without the measurements kept behind --full, and
--dump-outputs writes the last timed step's outputs, identical from run to
run (seeded weights, batch and noise).  The small T8 configuration keeps the
two runs to a few seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from _util import REPO  # noqa: E402


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--config', 'T8',
                        '--steps', '3', '--warmup', '2', '--dump-outputs', str(out_dir)],
                       timeout=200, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_last_step_outputs(gpu, tmp_path):
    rec = _plain_run(tmp_path / 'a')
    assert rec['steps'] == 3 and rec['warmup'] == 2 and rec['n_gpus'] == 1
    assert rec['unit'] == 'images/sec' and rec['higher_is_better'] is True and rec['dtype'] == 'bf16'
    assert rec['ms_per_step'] > 0
    # value and ms_per_step state the same time: 4 images (T8's batch) per step
    assert abs(rec['value'] - 4 / (rec['ms_per_step'] * 1e-3)) <= 2e-3 * rec['value']
    # what --full adds is absent, not zero
    assert rec['full'] is False and 'cpu_baseline' not in rec
    assert rec['host_submit_ms_per_step'] is None and rec['roofline']['achieved'] is None
    _plain_run(tmp_path / 'b')
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['fake_img_128.npy', 'fake_img_256.npy', 'fake_img_64.npy', 'g_loss.npy']
    assert sorted(os.listdir(tmp_path / 'b')) == names
    for n in names:
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        if n.startswith('fake_img'):
            s = int(n[len('fake_img_'):-len('.npy')])
            assert a.shape == (4, 3, s, s), (n, a.shape)
            assert np.abs(a).max() <= 1.0 and a.std() > 0     # tanh images, not a constant
        assert np.array_equal(a, b), n
