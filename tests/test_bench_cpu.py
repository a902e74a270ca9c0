"""bench.py's measurement plumbing on the CPU: `python bench.py --gpus N`
without a launcher starts an N-rank torch.distributed.run child job (one rank
per GPU, port bound by the store itself) and relays only rank 0's JSON line;
a rank whose job size differs from --gpus refuses to report."""
import json
import os
import subprocess
import sys

from _util import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_launcher_argv():
    argv = bench.launcher_argv(8, ['--gpus', '8', '--steps', '20', '--warmup', '5'])
    assert argv[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--standalone' in argv and argv[argv.index('--local-addr') + 1] == '127.0.0.1'
    assert argv[argv.index('--nproc-per-node') + 1] == '8'
    assert '--master-port' not in argv
    i = argv.index(os.path.join(REPO, 'bench.py'))
    assert argv[i + 1:] == ['--gpus', '8', '--steps', '20', '--warmup', '5']


def test_launch_ranks_relays_rank0_line(tmp_path, monkeypatch, capsys):
    script = tmp_path / 'fake_ranks.py'
    script.write_text('import json, sys\n'
                      'print("some rank chatter")\n'
                      'print(json.dumps({"metric": "m", "value": 1.5, "n_gpus": 2}))\n'
                      'sys.exit(int(sys.argv[1]))\n')
    monkeypatch.setattr(bench, 'launcher_argv', lambda n, argv: [sys.executable, str(script)] + list(argv))
    assert bench.launch_ranks(2, ['0']) == 0
    out, err = capsys.readouterr()
    assert [json.loads(x) for x in out.splitlines()] == [{'metric': 'm', 'value': 1.5, 'n_gpus': 2}]
    assert 'some rank chatter' in err
    assert bench.launch_ranks(2, ['3']) == 3           # the job's status is the launcher's


def test_dump_outputs_writes_float32_arrays(tmp_path):
    """--dump-outputs: the step's (fake_imgs, g_loss), bf16 images in NHWC
    storage behind their logical (B, 3, H, W) shape, land as float32 .npy
    files named by resolution, values unchanged."""
    import numpy as np
    import torch
    torch.manual_seed(0)
    imgs = [torch.randn(2, s, s, 8).to(torch.bfloat16)[..., :3].permute(0, 3, 1, 2) for s in (64, 128, 256)]
    g_loss = torch.tensor([1.25])
    d = tmp_path / 'out' / 'dump'
    bench.dump_outputs(str(d), (imgs, g_loss))
    assert sorted(os.listdir(d)) == ['fake_img_128.npy', 'fake_img_256.npy', 'fake_img_64.npy', 'g_loss.npy']
    total = 0
    for im in imgs:
        a = np.load(d / ('fake_img_%d.npy' % im.shape[-1]))
        assert a.dtype == np.float32 and a.shape == tuple(im.shape) and a.flags['C_CONTIGUOUS']
        assert np.array_equal(a, im.float().numpy())
        total += a.nbytes
    g = np.load(d / 'g_loss.npy')
    assert g.dtype == np.float32 and g.tolist() == [1.25]
    assert total + g.nbytes < 64e6


def test_op_log_needs_full():
    """--op-log records the timing pass, which only --full runs: a plain run
    given it stops at the command line instead of writing nothing."""
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--op-log', 'ops.json'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--full' in r.stderr
    assert not os.path.exists('ops.json')


def test_rank_refuses_mismatched_world(tmp_path):
    """A rank started with --gpus 2 in a one-rank job (WORLD_SIZE=1) must not
    print a line for the wrong GPU count."""
    env = dict(os.environ, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0', EEGAN_DIST_BACKEND='gloo')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '1'],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert 'refusing to report' in r.stderr
    assert not any(l.startswith('{') for l in r.stdout.splitlines())
