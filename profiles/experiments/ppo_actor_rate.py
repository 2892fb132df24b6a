"""On-policy collection on the reach-ball engine: the fused stochastic policy (Engine.rollout_policy: the 10-64-64-16 policy net,
the categorical or Gaussian head, the log-probability record and the env cycle in one launch of T cycles) against the launches
the repository already had (rollout_qnet, rollout_actor) and against the torch-in-the-loop step (Categorical(logits=net(obs))
.sample() + log_prob + step), and gae() against the T-iteration torch loop it replaces; 65 536 envs x T = 256, noise on, full
record (obs, action, reward, done, result, logp), in ONE process.

Protocol: every arm is warmed up for `--warmup` seconds of back-to-back work (past the clock ramp that follows an idle gap), then
`--regions` timed regions per arm, the arms alternating; a region is `--launches` fused launches (or `--loops` torch loops of T
steps) between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and the
highest, as seconds per T cycles and env-steps/s; and ratios of the medians.

--parent-arms times only rollout_qnet and rollout_actor: run it once with the library of this tree and once with S2D_LIB
pointing at a build of the parent commit to compare the launches whose code moved into a header.

Prints one JSON object; profiles/r08/ppo_actor_rate.json holds a run.
    python profiles/experiments/ppo_actor_rate.py [--n 65536] [--T 256] [--regions 5] [out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402

from soccer2d_amd.actor import DeterministicActor, QNetActor  # noqa: E402
from soccer2d_amd.engine import Engine, make_config  # noqa: E402

TASK = dict(change_ball_position=True, change_ball_velocity=True, min_distance_to_ball=5.0, max_steps=200, action_space_size=16)


def region(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count


def warm(fn, seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def mlp(a, act):
    return torch.nn.Sequential(torch.nn.Linear(10, 64), act(), torch.nn.Linear(64, 64), act(), torch.nn.Linear(64, a)).cuda()


def engine(n, continuous):
    e = Engine(n, 'cuda:0', cfg=make_config(noise=True, use_continuous_action=continuous, use_turning=False, **TASK))
    e.reset()
    return e


def gae_torch_loop(reward, done, value, last_value, gamma, lam, result, tval, adv, ret):
    """SB3's compute_returns_and_advantage as a learner writes it in torch: T iterations of small elementwise launches"""
    T = reward.shape[0]
    r = reward + gamma * tval * (result == 3)
    nt = 1.0 - done.float()
    next_v, last = last_value, torch.zeros_like(last_value)
    for t in range(T - 1, -1, -1):
        delta = r[t] + gamma * next_v * nt[t] - value[t]
        last = delta + gamma * lam * nt[t] * last
        adv[t] = last
        next_v = value[t]
    torch.add(adv, value, out=ret)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--T', type=int, default=256)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--launches', type=int, default=12)
    ap.add_argument('--loops', type=int, default=2)
    ap.add_argument('--warmup', type=float, default=1.0)
    ap.add_argument('--parent-arms', action='store_true')
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    n, T = a.n, a.T
    if not torch.cuda.is_available():
        raise SystemExit('ppo_actor_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    res = {'device': torch.cuda.get_device_name(0), 'n': n, 'T': T, 'net': '10-64-64-16 (10-64-64-1 continuous)', 'noise': True,
           'library': os.environ.get('S2D_LIB', 'this tree'),
           'protocol': {'regions': a.regions, 'fused_launches_per_region': a.launches, 'torch_loops_per_region': a.loops,
                        'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    relu, tanh = torch.nn.ReLU, torch.nn.Tanh
    arms, names = [], {}

    e_q = engine(n, False)
    q_actor = QNetActor.from_module(mlp(16, relu), epsilon=0.05)
    out_q = e_q.alloc_rollout(T)
    arms.append(('rollout_qnet', lambda: e_q.rollout_qnet(T, q_actor, out=out_q), a.launches))
    e_a = engine(n, True)
    d_actor = DeterministicActor.from_module(torch.nn.Sequential(*mlp(1, relu), torch.nn.Tanh()), epsilon=0.0, noise_sigma=0.1)
    out_a = e_a.alloc_rollout(T)
    arms.append(('rollout_actor_gauss', lambda: e_a.rollout_actor(T, d_actor, out=out_a), a.launches))

    if not a.parent_arms:
        from soccer2d_amd.actor import StochasticActor
        from soccer2d_amd.gae import gae
        e_r, e_t, e_c, e_s = engine(n, False), engine(n, False), engine(n, True), engine(n, False)
        p_relu, p_tanh = StochasticActor.from_module(mlp(16, relu)), StochasticActor.from_module(mlp(16, tanh))
        p_cont = StochasticActor.from_module(mlp(1, tanh), log_std=-0.5)
        out_r, out_t, out_c = (e.alloc_rollout(T, logp=True) for e in (e_r, e_t, e_c))
        arms += [('policy_discrete_relu', lambda: e_r.rollout_policy(T, p_relu, out=out_r), a.launches),
                 ('policy_discrete_tanh', lambda: e_t.rollout_policy(T, p_tanh, out=out_t), a.launches),
                 ('policy_continuous_tanh', lambda: e_c.rollout_policy(T, p_cont, out=out_c), a.launches)]
        net = mlp(16, tanh)
        rec = e_s.alloc_rollout(T, logp=True)

        def torch_loop():
            with torch.no_grad():
                obs = e_s.obs
                for t in range(T):
                    d = torch.distributions.Categorical(logits=net(obs))
                    act = d.sample()
                    rec['logp'][t] = d.log_prob(act)
                    obs, rew, done, result = e_s.step(act)
                    rec['obs'][t], rec['action'][t], rec['reward'][t], rec['done'][t], rec['result'][t] = obs, act, rew, done, result
        arms.append(('torch_in_the_loop_step', torch_loop, a.loops))

        e_r.rollout_policy(T, p_relu, out=out_r)
        torch.cuda.synchronize()
        value, tval = torch.randn((T, n), device='cuda:0'), torch.randn((T, n), device='cuda:0')
        last_value = torch.randn(n, device='cuda:0')
        reward, done, result = out_r['reward'].clone(), out_r['done'].clone(), out_r['result'].clone()
        g_out = (torch.empty((T, n), device='cuda:0'), torch.empty((T, n), device='cuda:0'))
        t_out = (torch.empty((T, n), device='cuda:0'), torch.empty((T, n), device='cuda:0'))
        arms += [('gae_kernel', lambda: gae(reward, done, value, last_value, 0.99, 0.95, result=result, terminal_value=tval, out=g_out),
                  a.launches),
                 ('gae_torch_loop', lambda: gae_torch_loop(reward, done, value, last_value, 0.99, 0.95, result, tval, *t_out), a.loops)]
        names = {'policy_discrete_relu': e_r, 'policy_discrete_tanh': e_t, 'policy_continuous_tanh': e_c}
    names.update({'rollout_qnet': e_q, 'rollout_actor_gauss': e_a})

    times = {name: [] for name, _, _ in arms}
    for name, fn, _ in arms:
        warm(fn, a.warmup)
    for _ in range(a.regions):
        for name, fn, count in arms:
            warm(fn, 0.1)                                  # back on this arm's code and clock after the other arms
            times[name].append(region(fn, count))
    for name, _, _ in arms:
        v = sorted(times[name])
        med = v[len(v) // 2]
        res[name] = {'seconds_per_T_cycles': {'median': med, 'min': v[0], 'max': v[-1], 'regions': times[name]},
                     'env_steps_per_s': {'median': n * T / med, 'min': n * T / v[-1], 'max': n * T / v[0]}}
        if name in names:
            res[name]['kernel'] = names[name].kernel_name()
    if not a.parent_arms:
        med = {name: res[name]['seconds_per_T_cycles']['median'] for name, _, _ in arms}
        res['speedup_policy_discrete_tanh_vs_torch_in_the_loop'] = med['torch_in_the_loop_step'] / med['policy_discrete_tanh']
        res['policy_discrete_relu_vs_rollout_qnet'] = med['policy_discrete_relu'] / med['rollout_qnet']
        res['policy_discrete_tanh_vs_relu'] = med['policy_discrete_tanh'] / med['policy_discrete_relu']
        res['policy_continuous_tanh_vs_rollout_actor_gauss'] = med['policy_continuous_tanh'] / med['rollout_actor_gauss']
        res['speedup_gae_kernel_vs_torch_loop'] = med['gae_torch_loop'] / med['gae_kernel']
        res['gae_kernel_bytes_per_s'] = n * T * 22 / med['gae_kernel']      # 4+1+4+1+4 read, 4+4 written per env-step
        got, want = g_out, t_out
        res['gae_max_abs_difference_kernel_vs_torch_loop'] = float(max((got[0] - want[0]).abs().max(), (got[1] - want[1]).abs().max()))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
