"""Rate of the fused epsilon-greedy Q-network actor (Engine.rollout_qnet) against the torch-in-the-loop step, in one process.

Configurations: 65 536 envs x T = 256, 10-64-64-16, eps = 0.05, full record + terminal observations, noise off; the same with
the lattice noise; the same at 4 096 envs; and the per-step API with a torch Q-network of the same shape in the loop (the recipe
of bench.py:measure_steps_with_policy).  Each figure is the median of `--repeats` timed graph replays after a settle phase.
Usage: python profiles/experiments/qnet_actor_rate.py [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'gym-soccer-2d-env_amd')):
    sys.path.insert(0, p)

import torch  # noqa: E402

from soccer2d_amd.actor import QNetActor  # noqa: E402
from soccer2d_amd.engine import Engine, make_config  # noqa: E402

DQN = dict(change_ball_position=True, change_ball_velocity=True, min_distance_to_ball=5.0, max_steps=200,
           use_continuous_action=False, action_space_size=16, use_turning=False)
PEAK_F32 = 157.3e12
FLOP_PER_STEP = 2 * (10 * 64 + 64 * 64 + 64 * 16)   # 11 520


def timed(fn, launches, repeats, settle_s=1.0):
    t_end = time.perf_counter() + settle_s
    while time.perf_counter() < t_end:
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    g.replay(); torch.cuda.synchronize()
    walls = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record(); b.synchronize()
        walls.append(a.elapsed_time(b) * 1e-3 / launches)
    walls.sort()
    return walls[len(walls) // 2], walls


def net_module():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                               torch.nn.Linear(64, 16)).to('cuda:0')


def fused(n, T, noise, repeats):
    eng = Engine(n, 'cuda:0', cfg=make_config(noise=noise, **DQN))
    eng.reset()
    actor = QNetActor.from_module(net_module(), epsilon=0.05)
    out = eng.alloc_rollout(T, terminal_obs=True)
    per, walls = timed(lambda: eng.rollout_qnet(T, actor, out=out), 2, repeats)
    return {'envs': n, 'T': T, 'noise': noise, 'us_per_launch': per * 1e6, 'env_steps_per_s': n * T / per,
            'flop_fraction_of_f32_peak': n * T * FLOP_PER_STEP / per / PEAK_F32, 'kernel': eng.kernel_name(),
            'repeats_us': [w * 1e6 for w in walls]}


def torch_loop(n, repeats):
    eng = Engine(n, 'cuda:0', cfg=make_config(noise=False, **DQN))
    eng.reset()
    net = net_module()

    def one():
        with torch.no_grad():
            eng.step(net(eng.obs).argmax(dim=1))
    per, walls = timed(one, 64, repeats)
    return {'envs': n, 'us_per_step': per * 1e6, 'env_steps_per_s': n / per, 'repeats_us': [w * 1e6 for w in walls],
            'policy': 'torch fp32 10-64-64-16 greedy, s2d_step, one hipGraph of 64 steps'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0)}
    res['fused_65536_T256_noise_off'] = fused(65536, 256, False, a.repeats)
    res['fused_65536_T256_lattice'] = fused(65536, 256, True, a.repeats)
    res['fused_4096_T256_noise_off'] = fused(4096, 256, False, a.repeats)
    res['torch_in_the_loop_65536'] = torch_loop(65536, a.repeats)
    res['speedup_fused_vs_torch_loop'] = (res['fused_65536_T256_noise_off']['env_steps_per_s'] /
                                          res['torch_in_the_loop_65536']['env_steps_per_s'])
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
