"""bench.py's harness: `--steps` validation, `--dump-outputs` (what the last timed step computed, as .npy files) and
`--full` (everything beside the headline figure).  The snapshot logic runs on the CPU with a stand-in step; the
end-to-end runs need the GPU."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_snapshot_outputs_names_dtypes_and_fixed_sample():
    """Every output comes back as float32; arrays above DUMP_MAX_ELEMS are sampled at the same sorted, distinct positions
    on every call (one per block), smaller ones keep their shape and values; the total stays under 64 MB."""
    bench = _bench()
    big = bench.DUMP_MAX_ELEMS * 3 + 7          # < 2^24: the float32 arange below holds every position exactly
    g = torch.Generator().manual_seed(1)
    hard = torch.randint(-1, 6, (2, 64, 64), generator=g)
    step = SimpleNamespace(last_hard=hard, prototypes=torch.randn(6, 2048, generator=g),
                           model=SimpleNamespace(flat_p=torch.arange(big, dtype=torch.float32)),
                           teacher=SimpleNamespace(flat_p=-torch.arange(big, dtype=torch.float32)))
    out = (torch.tensor([1.5]), torch.tensor([0.25]), torch.tensor([1e4]))
    a = bench.snapshot_outputs(step, out)
    assert set(a) == {'loss_source', 'loss_target', 'grad_norm_sq', 'pseudo_labels', 'prototypes', 'weights_sample',
                      'ema_weights_sample'}
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.array_equal(a['pseudo_labels'], hard.numpy().astype(np.float32))
    assert a['loss_source'].tolist() == [1.5] and a['grad_norm_sq'].tolist() == [1e4]
    pos = a['weights_sample'].astype(np.int64)       # flat_p = arange: the values are the sampled positions
    assert pos.size == bench.DUMP_MAX_ELEMS and np.all(np.diff(pos) > 0) and pos[-1] < big
    assert np.array_equal(a['ema_weights_sample'], -a['weights_sample'])
    b = bench.snapshot_outputs(step, out)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    step.teacher = None         # offline soft labels: no EMA shadow
    assert 'ema_weights_sample' not in bench.snapshot_outputs(step, out)


def test_steps_below_one_is_an_error():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and '--steps' in r.stderr


def test_full_is_off_by_default_and_names_the_record(monkeypatch):
    """A plain command line leaves `--full` off and writes no full record; `--full` sends the record to
    bench_out/bench_full.json next to the script unless `--full-json` names another place (which also holds without
    `--full`)."""
    bench = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '5', '--warmup', '2'])
    a = bench.parse()
    assert a.full is False and a.full_json is None and (a.steps, a.warmup, a.gpus) == (5, 2, 1)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full'])
    a = bench.parse()
    assert a.full is True and a.full_json == os.path.join(ROOT, 'bench_out', 'bench_full.json')
    for extra in ([], ['--full']):
        monkeypatch.setattr(sys, 'argv', ['bench.py', '--full-json', 'x.json'] + extra)
        assert bench.parse().full_json == 'x.json'


def test_plain_line_holds_the_contract_keys_only():
    """The line of a plain run: every contract key, none of the figures that `--full` measures, no record file."""
    bench = _bench()
    res = {'metric': 'm', 'value': 450.123456, 'unit': 'pairs/s', 'n_gpus': 1, 'steps': 10, 'warmup': 3,
           'ms_per_step': 17.7654321, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'bf16',
           'with_h2d_staging': None, 'comm_exposed_ms': None, 'replicas': None, 'ms_per_step_windows': [17.7654321]}
    line = bench.compact_line(res, None)
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup'):
        assert k in line
    assert line['value'] == 450.1 and line['ms_per_step'] == 17.77 and line['full_record'] is None
    for k in ('roofline', 'cpu_baseline', 'with_h2d_staging_pairs_per_s', 'host_enqueue_ms_per_step'):
        assert k not in line


@pytest.mark.gpu
def test_bench_plain_and_full(tmp_path):
    """The same command line without and with `--full`.  Plain: the contract keys, no roofline / CPU baseline / staging /
    enqueue figures, and nothing written.  `--full`: all of those, and the record file with the further windows."""
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1']
    lines = {}
    for name, extra in (('plain', []), ('full', ['--full', '--full-json', str(tmp_path / 'full.json')])):
        r = subprocess.run(cmd + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[name] = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
        if name == 'plain':
            assert not list(tmp_path.iterdir())
    moved = ('roofline', 'cpu_baseline', 'with_h2d_staging_pairs_per_s', 'host_enqueue_ms_per_step')
    for name, line in lines.items():
        assert line['metric'] == 'src+tgt 512x512 image-pairs/sec (SSL step)' and line['unit'] == 'pairs/s'
        assert line['higher_is_better'] is True and line['dtype'] == 'bf16' and line['steps'] == 2 and line['warmup'] == 1
        assert line['ms_per_step'] > 0 and line['plan_replay']
        assert abs(line['value'] * line['ms_per_step'] / 8e3 - 1) < 2e-3      # both rounded to 4 digits in the line
        assert all((k in line) == (name == 'full') for k in moved), (name, sorted(line))
    assert lines['plain']['full_record'] is None
    full = json.load(open(tmp_path / 'full.json'))
    assert len(full['ms_per_step_windows']) == 3 and full['ms_per_step_windows'][0] == full['ms_per_step']
    assert full['roofline']['by_kernel'] and full['cpu_baseline']['value'] > 0


@pytest.mark.gpu
def test_bench_dump_outputs(tmp_path):
    """`bench.py --steps 2 --dump-outputs DIR` on the recorded-plan path: the line reports the 2 steps and their
    ms_per_step, DIR holds the last timed step's outputs as float32 .npy files (< 64 MB), the losses finite."""
    dump = tmp_path / 'dump'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--repeats', '0',
           '--no-cpu-baseline', '--no-roofline', '--no-h2d', '--full-json', str(tmp_path / 'full.json'),
           '--dump-outputs', str(dump)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert res['steps'] == 2 and res['ms_per_step'] > 0 and res['plan_replay']
    files = sorted(p.name for p in dump.iterdir())
    assert files == sorted(['loss_source.npy', 'loss_target.npy', 'grad_norm_sq.npy', 'pseudo_labels.npy',
                            'prototypes.npy', 'weights_sample.npy', 'ema_weights_sample.npy'])
    a = {f[:-4]: np.load(dump / f) for f in files}
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a['pseudo_labels'].shape == (8, 512, 512) and a['pseudo_labels'].min() >= -1 and a['pseudo_labels'].max() < 6
    full = json.load(open(tmp_path / 'full.json'))      # the losses the record reports are those of the same step
    assert float(a['loss_source'].reshape(-1)[0]) == full['loss_source'] and np.isfinite(full['loss_source'])
    assert float(a['loss_target'].reshape(-1)[0]) == full['loss_target'] and np.isfinite(full['loss_target'])
    assert a['weights_sample'].size == _bench().DUMP_MAX_ELEMS and np.isfinite(a['weights_sample']).all()
