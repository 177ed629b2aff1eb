"""bench.py's plain run and ``--dump-outputs``: a run without ``--full``
times the steps only (the round-trip, sustained and comparison fields stay
null), ``--steps`` sets the timed steps, and the dump holds the last timed
step's replies as float .npy files: every request of the batch answered
with its node's czxid and data length, the sampled payloads as long as the
replies say."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_last_step(gpu, tmp_path):
    steps, batch, nodes, data = 3, 4096, 2000, 40
    d = str(tmp_path / 'out')
    out = subprocess.run(
        [sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps),
         '--warmup', '1', '--batch', str(batch), '--nodes', str(nodes),
         '--data-bytes', str(data), '--dump-outputs', d],
        cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
        timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec['steps'] == steps and rec['ms_per_step'] > 0
    assert rec['value'] == pytest.approx(
        batch / (rec['ms_per_step'] * 1e-3), rel=1e-6)
    # nothing but the timed steps ran
    for k in ('sustained', 'p50_get_rtt_us', 'p50_get_rtt_us_fakezk',
              'bulk_tcp_ops_s', 'end_to_end_ops_s', 'replica_value',
              'sharded_value'):
        assert rec[k] is None, k
    files = sorted(os.listdir(d))
    assert files and all(f.endswith('.npy') for f in files)
    arrs = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) < 64 << 20
    assert arrs['checked_ok'].tolist() == [steps * batch]
    conns = sorted({k.split('_')[0] for k in arrs if k.startswith('conn')})
    assert conns == ['conn0', 'conn1']               # --streams 2
    total = 0
    for c in conns:
        n = int(arrs[c + '_count'][0])
        total += n
        row = arrs[c + '_row']
        assert len(row) == n and (np.diff(row) > 0).all()    # all of them
        assert (arrs[c + '_err'] == 0).all()
        assert (arrs[c + '_status'] == 0).all()
        assert (arrs[c + '_pay_len'] == data).all()
        assert (arrs[c + '_dataLength'] == data).all()
        # leaves are nodes 1 + ndirs ..; node v has czxid v + 1
        cz = arrs[c + '_czxid']
        assert cz.min() >= 1 + 2 + 1 and cz.max() <= 1 + 2 + nodes
        assert len(np.unique(cz)) > n // 4           # a random batch
        pay = arrs[c + '_payload']
        assert pay.shape == (n, data)
        assert pay.min() >= 0 and pay.max() <= 255
        assert len(np.unique(pay)) > 200             # random bytes
    assert total == batch
