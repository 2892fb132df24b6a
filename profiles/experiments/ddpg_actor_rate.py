"""Rate of the fused tanh actor (Engine.rollout_actor) against the torch-in-the-loop DDPG step, in one process.

Configurations at 65 536 envs x T = 256, full record + terminal observations, eps = 0: 10-64-64-1 (continuous) and 10-64-64-4
(turning), noise off and lattice, each without and with Gaussian action noise (sigma = 0.1); rollout_qnet 10-64-64-16 at the
same size; and the per-step API with a torch 10-64-64-A tanh actor plus Gaussian noise in the loop.  Each figure is the median
of `--repeats` timed graph replays after a settle phase (the recipe of qnet_actor_rate.py).
Usage: python profiles/experiments/ddpg_actor_rate.py [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'gym-soccer-2d-env_amd'), os.path.join(ROOT, 'profiles', 'experiments')):
    sys.path.insert(0, p)

import torch  # noqa: E402

from qnet_actor_rate import fused as qnet_fused, timed  # noqa: E402
from soccer2d_amd.actor import DeterministicActor  # noqa: E402
from soccer2d_amd.engine import Engine, make_config  # noqa: E402

KW = dict(change_ball_position=True, change_ball_velocity=True, min_distance_to_ball=5.0, max_steps=200,
          use_continuous_action=True, action_space_size=16)


def mu_module(a):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                               torch.nn.Linear(64, a), torch.nn.Tanh()).to('cuda:0')


def fused(n, T, a, noise, sigma, repeats):
    eng = Engine(n, 'cuda:0', cfg=make_config(noise=noise, use_turning=a == 4, **KW))
    eng.reset()
    actor = DeterministicActor.from_module(mu_module(a), epsilon=0.0, noise_sigma=sigma)
    out = eng.alloc_rollout(T, terminal_obs=True)
    per, walls = timed(lambda: eng.rollout_actor(T, actor, out=out), 2, repeats)
    return {'envs': n, 'T': T, 'A': a, 'noise': noise, 'sigma': sigma, 'us_per_launch': per * 1e6,
            'env_steps_per_s': n * T / per, 'kernel': eng.kernel_name(), 'repeats_us': [w * 1e6 for w in walls]}


def torch_loop(n, a, repeats):
    eng = Engine(n, 'cuda:0', cfg=make_config(noise=False, use_turning=a == 4, **KW))
    eng.reset()
    net = mu_module(a)

    def one():
        with torch.no_grad():
            act = net(eng.obs)
            eng.step((act + 0.1 * torch.randn_like(act)).clamp(-1, 1))
    per, walls = timed(one, 64, repeats)
    return {'envs': n, 'A': a, 'us_per_step': per * 1e6, 'env_steps_per_s': n / per, 'repeats_us': [w * 1e6 for w in walls],
            'policy': f'torch fp32 10-64-64-{a} tanh + N(0, 0.1) noise, clamp, s2d_step, one hipGraph of 64 steps'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=256)
    o = ap.parse_args()
    n, T = o.envs, o.steps
    res = {'device': torch.cuda.get_device_name(0)}
    for a, name in ((1, 'cont1'), (4, 'turn4')):
        for noise in (False, True):
            for sigma in (None, 0.1):
                key = f"fused_{name}_{n}_T{T}_{'lattice' if noise else 'noise_off'}_{'gauss' if sigma else 'no_action_noise'}"
                res[key] = fused(n, T, a, noise, sigma, o.repeats)
        res[f'torch_in_the_loop_{name}_{n}'] = torch_loop(n, a, o.repeats)
        res[f'speedup_{name}_fused_gauss_vs_torch_loop'] = (res[f'fused_{name}_{n}_T{T}_noise_off_gauss']['env_steps_per_s'] /
                                                           res[f'torch_in_the_loop_{name}_{n}']['env_steps_per_s'])
    res[f'qnet_{n}_T{T}_noise_off'] = qnet_fused(n, T, False, o.repeats)
    text = json.dumps(res, indent=1)
    print(text)
    if o.out:
        os.makedirs(os.path.dirname(o.out) or '.', exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
