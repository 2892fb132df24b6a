"""11v11 collection on belief rows: the fused belief-network rollout (MatchEngine.set_network with a belief actor +
rollout(logp=True, net_index=True, belief_obs='all'): see rows, the belief update of all 22 rows, the 192-64-64-16 network on the
belief rows, its head, the body cycle and the vision step in one launch of T = 64 cycles) against what it replaces, in the same
process.  8192 matches, all 22 slots on the network, noise on.

  belief_policy_tanh / _relu   the belief policy launch, recording belief rows, indices and logp.
  belief_q_network             the belief Q launch at epsilon 0.1, recording belief rows and indices.
  see_policy_tanh              the see policy launch of the same shape (see rows, indices, logp): what the in-kernel update costs.
  see_policy_then_scan         that launch followed by belief_scan over its see record (flags: the done record shifted by one
                               row), the belief after every row recorded: the learner's path of INTEGRATION 5i.
  unfused_torch_loop           see -> belief_step -> the same torch module -> torch Categorical -> rollout(1) -> vision_step.

Protocol (profiles/experiments/match_see_net_rate.py's, whose helpers this script uses): every arm is warmed up for `--warmup`
seconds of back-to-back work, then `--regions` timed regions per arm, the arms alternating; a region is `--launches` fused launches
(or `--loops` unfused loops of T cycles) between two host clocks that end in a device synchronise.  Reported per arm: the median
region, the lowest and the highest, as seconds per T cycles, match-steps/s and agent decisions/s; and the ratios of the medians.
The shader clock is sampled with `rocm-smi --showclocks` (read only) while the belief tanh arm runs.  No rate here is a pass
condition.

Prints one JSON object; profiles/r23/match_belief_net_rate.json holds a run.
    python profiles/experiments/match_belief_net_rate.py [--n 8192] [--T 64] [--regions 5] [out.json]"""
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


def engine(n, actor=None, belief=False):
    eng = MatchEngine(n, 'cuda:0', noise=True)
    eng.enable_vision()
    if belief:
        eng.enable_belief('all')
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
    ap.add_argument('--loops', type=int, default=6)
    ap.add_argument('--warmup', type=float, default=1.0)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    n, T = a.n, a.T
    if not torch.cuda.is_available():
        raise SystemExit('match_belief_net_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    table = torch.stack([torch.randint(1, 5, (K,), generator=g).float(), torch.rand(K, generator=g) * 200 - 100,
                         torch.rand(K, generator=g) * 360 - 180, torch.rand(K, generator=g) * 120 - 60,
                         torch.randint(0, 4, (K,), generator=g).float()], dim=1)
    pi = {'tanh': module(torch.nn.Tanh), 'relu': module(torch.nn.ReLU)}
    res = {'device': torch.cuda.get_device_name(0), 'n': n, 'T': T, 'net': f'192-64-64-{K}', 'slots': 22, 'noise': True,
           'records': 'belief rows of all 22 slots, net_index, logp (Q arm: no logp; see policy arms: see rows in their place)',
           'protocol': {'regions': a.regions, 'fused_launches_per_region': a.launches, 'unfused_loops_per_region': a.loops,
                        'warmup_seconds': a.warmup, 'arms': 'alternating'}, 'kernels': {}}
    arms, engines = [], []
    for act in ('tanh', 'relu'):
        eng = engine(n, MatchSeePolicyActor.from_module(pi[act], table, obs='belief'), belief=True)
        out = eng.alloc_rollout(T, with_obs=False)
        engines.append(eng)
        res['kernels'][f'belief_policy_{act}'] = eng.kernel_name()
        arms.append((f'belief_policy_{act}',
                     lambda eng=eng, out=out: eng.rollout(T, out=out, with_obs=False, logp=True, net_index=True, belief_obs='all'),
                     a.launches))
    qeng = engine(n, MatchQNetActor.from_module(pi['relu'], table, epsilon=EPS, obs='belief'), belief=True)
    qout = qeng.alloc_rollout(T, with_obs=False)
    engines.append(qeng)
    res['kernels']['belief_q_network'] = qeng.kernel_name()
    arms.append(('belief_q_network', lambda: qeng.rollout(T, out=qout, with_obs=False, net_index=True, belief_obs='all'), a.launches))

    seng = engine(n, MatchSeePolicyActor.from_module(pi['tanh'], table))
    sout = seng.alloc_rollout(T, with_obs=False)
    engines.append(seng)
    res['kernels']['see_policy_tanh'] = seng.kernel_name()
    arms.append(('see_policy_tanh', lambda: seng.rollout(T, out=sout, with_obs=False, logp=True, net_index=True, see_obs='all'),
                 a.launches))

    beng = engine(n, MatchSeePolicyActor.from_module(pi['tanh'], table), belief=True)
    bout = beng.alloc_rollout(T, with_obs=False)
    brec = torch.empty((T, n, 22, 192), device='cuda:0')
    flags = torch.zeros((T, n), dtype=torch.uint8, device='cuda:0')
    engines.append(beng)

    def then_scan():
        flags[0] = beng.done                               # (the done plane before the launch: the cycle before its first row)
        beng.rollout(T, out=bout, with_obs=False, logp=True, net_index=True, see_obs='all')
        flags[1:] = bout['done'][:T - 1]
        beng.belief_scan(bout['see'], reset=flags, out=brec)

    arms.append(('see_policy_then_scan', then_scan, a.launches))

    loose = engine(n, belief=True)
    engines.append(loose)
    ro = loose.alloc_rollout(1, with_obs=False)
    rows = torch.empty((n, 22, 192), device='cuda:0')
    tab = table.cuda()

    def unfused():
        with torch.no_grad():
            for _ in range(T):
                x = loose.belief_step(loose.see('all', out=rows), done=True)
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
            if name == 'belief_policy_tanh':
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
    for name in ('belief_policy_tanh', 'belief_policy_relu', 'belief_q_network'):
        res[f'{name}_time_vs_see_policy_tanh'] = med[name] / med['see_policy_tanh']
        res[f'{name}_time_vs_see_policy_then_scan'] = med[name] / med['see_policy_then_scan']
        res[f'speedup_{name}_vs_unfused'] = med['unfused_torch_loop'] / med[name]
    s = sorted(clock.samples)
    res['shader_clock_mhz_during_belief_policy_tanh'] = ({'median': s[len(s) // 2], 'min': s[0], 'max': s[-1], 'samples': len(s)} if s
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
