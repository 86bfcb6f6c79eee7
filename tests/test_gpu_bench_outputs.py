"""A plain `bench.py --gpus 1` run: the headline line alone (the other measurements and checks
run only with --full), --steps timed steps, and --dump-outputs writing what the last timed step
returned - the same arrays from run to run, since the inputs are seeded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SMALL = ['--gpus', '1', '--rois', '256', '--height', '160', '--width', '256', '--steps', '3',
         '--warmup', '1']


def _bench(*argv):
    e = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if bench.is_result_line(l)]
    assert r.returncode == 0 and lines, r.stderr[-4000:]
    return json.loads(lines[-1])


def test_plain_run_times_its_steps_and_dumps_the_last_steps_outputs(dev, tmp_path):
    runs = []
    for i in range(2):
        d = str(tmp_path / ('run%d' % i))
        res = _bench(*SMALL, '--dump-outputs', d)
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in res, k
        assert res['steps'] == 3 and res['ms_per_step'] > 0 and res['value'] > 0
        for k in ('cpu_baseline', 'fp32x3_plan', 'fp32_mfma_plan', 'parity_in_run', 'bf16_c80_plan',
                  'tta_infer', 'scaling_baseline_value'):
            assert k not in res, k
        assert res['config']['deferred_route_ms_per_step'] is None
        assert not any(k.startswith('projected_') for k in res['config'])
        runs.append({f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))})
    a, b = runs
    assert sorted(a) == sorted(b)
    for k in ('loss_cls', 'loss_cls_noise', 'logits', 'd_logits', 'cls_prob', 'params_sample'):
        assert k in a, k
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    assert a['loss_cls'].shape == (2,) and a['logits'].shape == a['d_logits'].shape
    assert a['params_sample'].size > 1000000 - 10000
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.isfinite(a[k]).all(), k
        assert np.allclose(a[k], b[k], rtol=1e-5, atol=1e-7), k
