"""Rate of the fused Q-network actor on a general MLP (Engine.rollout_qnet with an MlpQNetActor) against the two-layer actor and
against the torch-in-the-loop step, in one process.  The protocol of qnet_actor_rate.py: 65 536 envs x T = 256, eps = 0.05, full
record + terminal observations, noise off; every arm is one captured graph, timed `--repeats` times with the arms ALTERNATED
(one replay of each per round), the figure is the median.

  a  rollout_qnet, QNetActor 10-64-64-16 (ReLU)                     the two-layer kernel
  b  rollout_qnet, MlpQNetActor on the same network                 b / a = the price of the general layer loop
  c  rollout_qnet, MlpQNetActor 10-128-64-32-16-16 Tanh             the reference's custom DQN model
  d  s2d_step with c's torch module in the loop (one graph of 64 steps)

Usage: python profiles/experiments/mlp_actor_rate.py [--repeats 7] [--out FILE]"""
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
from soccer2d_amd.mlp_actor import MlpQNetActor  # noqa: E402

DQN = dict(change_ball_position=True, change_ball_velocity=True, min_distance_to_ball=5.0, max_steps=200,
           use_continuous_action=False, action_space_size=16, use_turning=False)
N, T, LOOP_STEPS = 65536, 256, 64


def module(hidden, act):
    torch.manual_seed(0)
    layers, win = [], 10
    for w in hidden:
        layers += [torch.nn.Linear(win, w), act()]
        win = w
    layers.append(torch.nn.Linear(win, 16))
    return torch.nn.Sequential(*layers).to('cuda:0')


def capture(fn, launches, settle_s=1.0):
    t_end = time.perf_counter() + settle_s
    while time.perf_counter() < t_end:
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    g.replay(); torch.cuda.synchronize()
    return g


def fused_arm(actor):
    eng = Engine(N, 'cuda:0', cfg=make_config(noise=False, **DQN))
    eng.reset()
    out = eng.alloc_rollout(T, terminal_obs=True)
    g = capture(lambda: eng.rollout_qnet(T, actor, out=out), 2)
    return dict(graph=g, launches=2, steps=N * T, keep=(eng, actor, out), kernel=eng.kernel_name())


def loop_arm(net):
    eng = Engine(N, 'cuda:0', cfg=make_config(noise=False, **DQN))
    eng.reset()

    def one():
        with torch.no_grad():
            eng.step(net(eng.obs).argmax(dim=1))
    g = capture(one, LOOP_STEPS)
    return dict(graph=g, launches=LOOP_STEPS, steps=N, keep=(eng, net), kernel='s2d_step + torch fp32 forward, greedy')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    two, deep = module((64, 64), torch.nn.ReLU), module((128, 64, 32, 16), torch.nn.Tanh)
    arms = {'a_two_layer_10-64-64-16': fused_arm(QNetActor.from_module(two, epsilon=0.05)),
            'b_mlp_10-64-64-16': fused_arm(MlpQNetActor.from_module(two, epsilon=0.05)),
            'c_mlp_10-128-64-32-16-16_tanh': fused_arm(MlpQNetActor.from_module(deep, epsilon=0.05)),
            'd_torch_in_the_loop_10-128-64-32-16-16_tanh': loop_arm(deep)}
    walls = {k: [] for k in arms}
    for _ in range(a.repeats):
        for k, arm in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); arm['graph'].replay(); e1.record(); e1.synchronize()
            walls[k].append(e0.elapsed_time(e1) * 1e-3 / arm['launches'])
    res = {'device': torch.cuda.get_device_name(0), 'envs': N, 'T': T, 'epsilon': 0.05, 'repeats': a.repeats}
    for k, arm in arms.items():
        w = sorted(walls[k])
        per = w[len(w) // 2]
        res[k] = {'us_per_launch': per * 1e6, 'env_steps_per_s': arm['steps'] / per, 'kernel': arm['kernel'],
                  'repeats_us': [v * 1e6 for v in w]}
    rate = lambda k: res[k]['env_steps_per_s']  # noqa: E731
    res['b_over_a'] = rate('b_mlp_10-64-64-16') / rate('a_two_layer_10-64-64-16')
    res['c_over_d'] = rate('c_mlp_10-128-64-32-16-16_tanh') / rate('d_torch_in_the_loop_10-128-64-32-16-16_tanh')
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
