"""11v11 on-policy collection under partial observability: the fused see-policy rollout (MatchEngine.set_network with a
MatchSeePolicyActor + rollout(logp=True, net_index=True, see_obs='all'): see rows, the 192-64-64-16 policy, its categorical head,
the body cycle and the vision step of all 22 players in one launch of T = 64 cycles), once per hidden activation, against two
baselines in the same process: the see Q-network launch of the same shape with the same records (epsilon 0.1), and the unfused
cycle see('all') -> the same torch module -> torch Categorical (sample, log_prob) -> gather from the action table -> rollout(1)
-> vision_step.  8192 matches, all 22 slots on the policy, noise on.

Protocol (profiles/experiments/match_see_net_rate.py's, whose helpers this script uses): every arm is warmed up for `--warmup`
seconds of back-to-back work (past the clock ramp that follows an idle gap), then `--regions` timed regions per arm, the arms
alternating; a region is `--launches` fused launches (or `--loops` unfused loops of T cycles) between two host clocks that end in
a device synchronise.  Reported per arm: the median region, the lowest and the highest, as seconds per T cycles, match-steps/s
and agent decisions/s; and the ratios of the medians.  The shader clock is sampled with `rocm-smi --showclocks` while the fused
tanh arm runs (the clock the device grants under this load); "not measured" without it.  No rate here is a pass condition.

Prints one JSON object; profiles/r18/match_see_policy_rate.json holds a run.
    python profiles/experiments/match_see_policy_rate.py [--n 8192] [--T 64] [--regions 5] [out.json]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from match_see_net_rate import ClockSampler, region, warm  # noqa: E402
from soccer2d_amd.actor import MatchQNetActor, MatchSeePolicyActor  # noqa: E402
from soccer2d_amd.match import MatchEngine  # noqa: E402

EPS = 0.1
K = 16


def module(act):
    return torch.nn.Sequential(torch.nn.Linear(192, 64), act(), torch.nn.Linear(64, 64), act(), torch.nn.Linear(64, K)).cuda()


def engine(n, actor=None):
    eng = MatchEngine(n, 'cuda:0', noise=True)
    eng.enable_vision()
    if actor is not None:
        eng.set_network(actor)
    eng.reset()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--launches', type=int, default=12)
    ap.add_argument('--loops', type=int, default=12)
    ap.add_argument('--warmup', type=float, default=1.0)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    n, T = a.n, a.T
    if not torch.cuda.is_available():
        raise SystemExit('match_see_policy_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    table = torch.stack([torch.randint(1, 5, (K,), generator=g).float(), torch.rand(K, generator=g) * 200 - 100,
                         torch.rand(K, generator=g) * 360 - 180, torch.rand(K, generator=g) * 120 - 60,
                         torch.randint(0, 4, (K,), generator=g).float()], dim=1)
    pi = {'tanh': module(torch.nn.Tanh), 'relu': module(torch.nn.ReLU)}
    res = {'device': torch.cuda.get_device_name(0), 'n': n, 'T': T, 'net': f'192-64-64-{K}', 'slots': 22, 'noise': True,
           'records': 'see rows of all 22 slots, net_index, logp (the Q-network arm: see rows, net_index)',
           'protocol': {'regions': a.regions, 'fused_launches_per_region': a.launches, 'unfused_loops_per_region': a.loops,
                        'warmup_seconds': a.warmup, 'arms': 'alternating'}, 'kernels': {}}
    arms, engines = [], []
    for act in ('tanh', 'relu'):
        eng = engine(n, MatchSeePolicyActor.from_module(pi[act], table))
        out = eng.alloc_rollout(T, with_obs=False)
        engines.append(eng)
        res['kernels'][f'see_policy_{act}'] = eng.kernel_name()
        arms.append((f'see_policy_{act}',
                     lambda eng=eng, out=out: eng.rollout(T, out=out, with_obs=False, logp=True, net_index=True, see_obs='all'),
                     a.launches))
    qeng = engine(n, MatchQNetActor.from_module(pi['relu'], table, epsilon=EPS, obs='see'))
    qout = qeng.alloc_rollout(T, with_obs=False)
    engines.append(qeng)
    res['kernels']['see_q_network'] = qeng.kernel_name()
    arms.append(('see_q_network', lambda: qeng.rollout(T, out=qout, with_obs=False, net_index=True, see_obs='all'), a.launches))

    loose = engine(n)
    engines.append(loose)
    ro = loose.alloc_rollout(1, with_obs=False)
    rows = torch.empty((n, 22, 192), device='cuda:0')
    tab = table.cuda()

    def unfused():
        with torch.no_grad():
            for _ in range(T):
                x = loose.see('all', out=rows)
                d = torch.distributions.Categorical(logits=pi['tanh'](x))
                idx = d.sample()
                d.log_prob(idx)
                act = tab[idx]
                loose.rollout(1, actions=act[..., :3].unsqueeze(0), out=ro, with_obs=False)
                loose.vision_step(act[..., 3:], done=True)

    arms.append(('unfused_torch_loop', unfused, a.loops))
    times = {name: [] for name, _, _ in arms}
    clock = ClockSampler()
    for name, fn, _ in arms:
        warm(fn, a.warmup)
    for _ in range(a.regions):
        for name, fn, count in arms:
            warm(fn, 0.1)                                  # back on this arm's code and clock after the other arms
            if name == 'see_policy_tanh':
                with clock:
                    times[name].append(region(fn, count))
            else:
                times[name].append(region(fn, count))
    for name, _, _ in arms:
        v = sorted(times[name])
        med = v[len(v) // 2]
        res[name] = {'seconds_per_T_cycles': {'median': med, 'min': v[0], 'max': v[-1], 'regions': times[name]},
                     'match_steps_per_s': {'median': n * T / med, 'min': n * T / v[-1], 'max': n * T / v[0]},
                     'agent_decisions_per_s': {'median': 22 * n * T / med, 'min': 22 * n * T / v[-1], 'max': 22 * n * T / v[0]}}
    med = {name: res[name]['seconds_per_T_cycles']['median'] for name, _, _ in arms}
    for act in ('tanh', 'relu'):
        res[f'see_policy_{act}_time_vs_see_q_network'] = med[f'see_policy_{act}'] / med['see_q_network']
        res[f'speedup_see_policy_{act}_vs_unfused'] = med['unfused_torch_loop'] / med[f'see_policy_{act}']
    s = sorted(clock.samples)
    res['shader_clock_mhz_during_see_policy_tanh'] = ({'median': s[len(s) // 2], 'min': s[0], 'max': s[-1], 'samples': len(s)} if s
                                                      else 'not measured')
    for eng in engines:
        eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
