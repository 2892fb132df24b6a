"""examples/td3_reach_ball.py for a few hundred updates at 256 envs: with the fused actor, the fused target and the fused learner
(the two captured graphs of the delayed update) in both action modes, and once with none of them (torch in the loop).  Each run is
a fresh child process under its own timeout; it must exit 0, print the goal-share line and report finite losses."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'examples', 'td3_reach_ball.py')
FUSED = ['--fused-actor', '16', '--fused-target', '--fused-learner']


@pytest.mark.parametrize('flags', [FUSED, FUSED + ['--turning'], []], ids=['fused-cont1', 'fused-turn4', 'torch-cont1'])
def test_example_runs(tmp_path, flags):
    iters = 2
    r = subprocess.run([sys.executable, EXAMPLE, '--envs', '256', '--iters', str(iters), '--train-steps', '128', '--test-steps', '40',
                        '--batch', '256'] + flags, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    assert any(line.startswith('goal share: ') for line in lines), r.stdout[-3000:]
    losses = [[float(line.split(f' {name} ')[1].split()[0]) for name in ('loss_q', 'loss_pi')] for line in lines if ' loss_q ' in line]
    assert len(losses) == iters and np.isfinite(np.array(losses)).all(), r.stdout[-3000:]
    assert all(('captured graphs' in line) == bool(flags) for line in lines if ' loss_q ' in line), r.stdout[-3000:]
