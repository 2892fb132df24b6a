"""Rate of the GoToCenter fused actors (GoToCenterVecEnv.rollout_qnet / rollout_actor with the Gtc* actors) against the
torch-in-the-loop step with the same module and against the random-policy rollout, in one process.  The protocol of
wide_actor_rate.py: 65 536 envs, eps = 0.05, full record + terminal observations; every arm is one captured graph (the pack
kernel is in it), timed `--repeats` times after a warm-up with the arms ALTERNATED (one replay of each per round); the figure is
the median.  T is chosen so that a launch lasts a few ms: 256 for the small networks, 32 for [400] * 5.

  a  rollout_qnet, GtcQNetActor 4-64-64-16 ReLU (discrete env)                                   SB3's DQN default
  b  rollout_actor, GtcDeterministicActor [16, 8] ReLU, use_turn, A = 4, Gaussian noise          the script's DDPG actor
  c  rollout_qnet, GtcQNetActor [400] * 5 Sigmoid                                                 the Optuna grid's largest
  a' b' c'  step() with the same torch module in the loop (one graph of 16 steps)
  r  rollout(): the random policy, discrete env                                                   the ceiling

Usage: python profiles/experiments/gtc_actor_rate.py [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'gym-soccer-2d-env_amd')):
    sys.path.insert(0, p)

import torch  # noqa: E402

from soccer2d_amd.gtc import GoToCenterVecEnv  # noqa: E402
from soccer2d_amd.gtc_actor import GtcDeterministicActor, GtcQNetActor, gtc_plan  # noqa: E402

DISCRETE = dict(continuous=0)
USETURN = dict(continuous=1, turn=1, use_turn=1, actor_out_size=4)
N, LOOP_STEPS = 65536, 16
ACT = {'relu': torch.nn.ReLU, 'tanh': torch.nn.Tanh, 'sigmoid': torch.nn.Sigmoid}


def module(hidden, act, na=16, tanh_head=False):
    torch.manual_seed(0)
    layers, win = [], 4
    for w in hidden:
        layers += [torch.nn.Linear(win, w), ACT[act]()]
        win = w
    layers.append(torch.nn.Linear(win, na))
    if tanh_head:
        layers.append(torch.nn.Tanh())
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


def fused_arm(actor, T, task, launches=2):
    env = GoToCenterVecEnv(N, 'cuda:0', **task)
    env.reset()
    roll = env.rollout_actor if task is USETURN else env.rollout_qnet
    out = roll(T, actor, terminal_obs=True)
    g = capture(lambda: roll(T, actor, out=out), launches)
    return dict(graph=g, launches=launches, steps=N * T, T=T, keep=(env, actor, out), kernel=env.kernel_name())


def loop_arm(net, task):
    env = GoToCenterVecEnv(N, 'cuda:0', **task)
    env.reset()

    def one():
        with torch.no_grad():
            if task is USETURN:
                act = net(env.obs)
                env.step((act + 0.1 * torch.randn_like(act)).clamp(-1, 1))
            else:
                env.step(net(env.obs).argmax(dim=1))
    g = capture(one, LOOP_STEPS)
    return dict(graph=g, launches=LOOP_STEPS, steps=N, T=1, keep=(env, net), kernel='s2d_gtc_step + torch fp32 forward')


def random_arm(T, launches=2):
    env = GoToCenterVecEnv(N, 'cuda:0', **DISCRETE)
    env.reset()
    out = env._alloc_rollout(T, True)
    ro = env._rollout_struct(out)
    import ctypes as C

    def one():
        env.lib.s2d_gtc_rollout(env._h, T, C.byref(ro), env._stream())
    g = capture(one, launches)
    return dict(graph=g, launches=launches, steps=N * T, T=T, keep=(env, out, ro), kernel='s2d_gtc_rollout_kernel (random policy)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    small = module((64, 64), 'relu')
    ddpg = module((16, 8), 'relu', 4, tanh_head=True)
    deep = module((400,) * 5, 'sigmoid')
    shapes = {'a': ((64, 64), 16), 'b': ((16, 8), 4), 'c': ((400,) * 5, 16)}
    arms = {
        'a_fused_4-64-64-16_relu': fused_arm(GtcQNetActor.from_module(small, epsilon=0.05), 256, DISCRETE),
        'a_torch_in_the_loop': loop_arm(small, DISCRETE),
        'b_fused_actor_4-16-8-4_relu_useturn_gauss': fused_arm(GtcDeterministicActor.from_module(ddpg, epsilon=0.05, noise_sigma=0.1),
                                                               256, USETURN),
        'b_torch_in_the_loop': loop_arm(ddpg, USETURN),
        'c_fused_4-400x5-16_sigmoid': fused_arm(GtcQNetActor.from_module(deep, epsilon=0.05), 32, DISCRETE, launches=1),
        'c_torch_in_the_loop': loop_arm(deep, DISCRETE),
        'r_random_rollout': random_arm(256),
    }
    walls = {k: [] for k in arms}
    for _ in range(2):                                     # one untimed round of every arm behind the captures
        for arm in arms.values():
            arm['graph'].replay()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for k, arm in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); arm['graph'].replay(); e1.record(); e1.synchronize()
            walls[k].append(e0.elapsed_time(e1) * 1e-3 / arm['launches'])
    res = {'device': torch.cuda.get_device_name(0), 'envs': N, 'epsilon': 0.05, 'repeats': a.repeats}
    for k, arm in arms.items():
        w = sorted(walls[k])
        per = w[len(w) // 2]
        res[k] = {'T': arm['T'], 'us_per_launch': per * 1e6, 'env_steps_per_s': arm['steps'] / per, 'kernel': arm['kernel'],
                  'repeats_us': [v * 1e6 for v in w]}
        if '_fused' in k:
            waves, tiles, lds, ws = gtc_plan(*shapes[k[0]])
            res[k].update({'waves': waves, 'tiles': tiles, 'lds_bytes': lds, 'workspace_bytes': ws})
    rate = lambda k: res[k]['env_steps_per_s']  # noqa: E731
    for c, k in (('a', 'a_fused_4-64-64-16_relu'), ('b', 'b_fused_actor_4-16-8-4_relu_useturn_gauss'), ('c', 'c_fused_4-400x5-16_sigmoid')):
        res[f'{c}_over_torch'] = rate(k) / rate(f'{c}_torch_in_the_loop')
        res[f'{c}_over_random_rollout'] = rate(k) / rate('r_random_rollout')
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
