"""--episode-stats and --fused-eval in the examples: the scripts run to the end, print the new ep_rew_mean line per iteration and
keep the lines they printed before."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

EXAMPLES_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gym-soccer-2d-env_amd', 'examples')
STATS_LINE = r'iter (\d+): ep_rew_mean (\S+)  ep_len_mean (\S+)  Goal (\S+) over the last (\d+) of (\d+) training episodes'


def run(tmp_path, script, flags):
    r = subprocess.run([sys.executable, os.path.join(EXAMPLES_DIR, script)] + flags, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def stats_lines(out, iters):
    found = re.findall(STATS_LINE, out)
    assert [int(f[0]) for f in found] == list(range(iters)), out[-3000:]
    for _i, rew, length, goal, window, total in found:
        assert int(window) == min(int(total), 100)
        if int(total) == 0:                                          # no episode has ended yet: SB3 logs nothing, this line says nan
            assert rew == length == goal == 'nan'
        else:
            assert float(rew) == float(rew) and float(length) >= 1.0 and 0.0 <= float(goal) <= 1.0
    return found


def test_ppo_episode_stats_and_fused_eval(tmp_path):
    out = run(tmp_path, 'ppo_reach_ball.py', ['--envs', '256', '--iters', '2', '--train-steps', '32', '--test-steps', '40',
                                              '--fused-actor', '16', '--tanh', '--episode-stats', '--fused-eval', '20'])
    stats_lines(out, 2)
    assert re.search(r'goal share: \d\.\d{4} before, \d\.\d{4} after 2 iterations', out), out[-3000:]
    assert "untrained policy: {'Goal':" in out and "'ep_rew_mean':" in out        # the fused evaluation's dict: test()'s keys and more
    assert len(re.findall(r'iter \d: loss ', out)) == 2


def test_ppo_without_the_flags_prints_what_it_printed(tmp_path):
    out = run(tmp_path, 'ppo_reach_ball.py', ['--envs', '256', '--iters', '1', '--train-steps', '32', '--test-steps', '10',
                                              '--fused-actor', '16', '--tanh'])
    assert 'ep_rew_mean' not in out and 'goal share: ' in out
    assert re.search(r"untrained policy: \{'Goal': \S+, 'Out': \S+, 'Timeout': \S+, 'episodes': \d+\}\n", out), out[-3000:]


def test_dqn_episode_stats(tmp_path):
    out = run(tmp_path, 'dqn_reach_ball.py', ['--envs', '256', '--iters', '1', '--train-steps', '32', '--test-steps', '10',
                                              '--fused-actor', '16', '--episode-stats'])
    stats_lines(out, 1)
    assert 'random policy:' in out and re.search(r'iter 0: \S+ M env-steps/s incl\. learning', out), out[-3000:]
