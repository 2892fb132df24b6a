"""What the in-kernel agent reward (s2d_match_set_agent_reward, include/s2d_match.h) costs, at 8192 matches, T = 64 cycles per
launch, stock rules, noise on.  Arms of this commit's library, one process:

  policy / policy_reward            the policy launch (224-64-64-16 Tanh on all 22 slots, logp and net_index recorded) without
                                    and with the agent reward record
  controllers / controllers_reward  the controllers launch (scripted left, random right) without and with the record
  policy_rows                       the policy launch that also records agent_obs='all' ([T, N, 22, 224])
  unfused                           policy_rows, then agent_observations('all') for the rows after the last cycle and the same six
                                    terms and weighted sum in torch (no chaser gate; fp32, not bit-exact: torch has no fmaf chain)

and the condition on the unchanged paths: bench.py's secondary.match_8192 (`bench.py --task match --steps 16`, the same
measure_match call) on this tree and on a checkout of the parent commit built beside it (--parent-tree), the two alternating in
one session, each run a process of its own.

Protocol: every arm is warmed up for --warmup seconds of back-to-back launches, then --regions timed regions per arm, the arms
alternating; a region is --launches launches between two host clocks that end in a device synchronise.  Reported per arm: the
median, lowest and highest region as seconds per T cycles and match-steps/s, and the ratios of the medians.

Prints one JSON object; profiles/r05/match_agent_reward_rate.json holds a run.
    python profiles/experiments/match_agent_reward_rate.py --parent-tree PATH [--n 8192] [--T 64] [out.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))
WEIGHTS = (1.0, 0.03, 0.7, 0.3, 0.11, 0.05)
PLAY_ON, CARD_RED = 2, 2


def torch_reward(torch, rows, last, reward, w):
    """the six terms from the recorded start-of-cycle rows [T, N, 22, 224] and the rows after the last cycle [N, 22, 224]"""
    def pair(k):
        cur = rows[..., k]
        return cur, torch.cat([cur[1:], last[None, ..., k]])
    bx0, bx1 = pair(16)
    d0, d1 = pair(20)
    b0, b1 = pair(21)
    _t0, touch1 = pair(22)
    _k0, kick1 = pair(12)
    c0, c1 = pair(11)
    m0, m1 = pair(24)
    sign = torch.tensor([1.0] * 11 + [-1.0] * 11, device=rows.device)
    play1 = m1 == PLAY_ON
    live = (m0 == PLAY_ON) & play1
    active = (c0 < CARD_RED) & (c1 < CARD_RED)
    zero = torch.zeros_like(bx0)
    terms = (reward[:, :, None] * sign, torch.where(live, bx1 - bx0, zero), torch.where(live & active, d0 - d1, zero),
             torch.where(live & active, (b0.abs() - b1.abs()) * (1.0 / 180.0), zero), torch.where(play1 & active, kick1, zero),
             torch.where(play1, touch1, zero))
    acc = zero
    for k in range(6):
        acc = acc + w[k] * terms[k]
    return acc


def arms_of(n, T):
    import torch
    from soccer2d_amd.actor import MatchPolicyActor
    from soccer2d_amd.match import MatchEngine
    torch.manual_seed(0)
    pi = torch.nn.Sequential(torch.nn.Linear(224, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                             torch.nn.Linear(64, 16)).cuda()
    g = torch.Generator().manual_seed(1)
    table = torch.stack([torch.randint(1, 5, (16,), generator=g).float(), torch.rand(16, generator=g) * 200 - 100,
                         torch.rand(16, generator=g) * 360 - 180], dim=1)
    arms, names = {}, {}

    def engine(policy, reward):
        eng = MatchEngine(n, 'cuda:0', noise=True)
        if policy:
            eng.set_network(MatchPolicyActor.from_module(pi, table), 'all')
        else:
            eng.set_controllers({'left': 'scripted', 'right': 'random'})
        if reward:
            eng.set_agent_reward(WEIGHTS)
        eng.reset()
        return eng, eng.alloc_rollout(T, with_obs=False)

    def fused(name, policy, reward, **kw):
        eng, out = engine(policy, reward)
        if policy:
            kw.update(logp=True, net_index=True)
        arms[name] = lambda: eng.rollout(T, out=out, with_obs=False, agent_reward=reward, **kw)
        arms[name]()                                       # (allocates the records)
        names[name] = eng.kernel_name()
        return eng, out

    fused('policy', True, False)
    fused('policy_reward', True, True)
    fused('controllers', False, False)
    fused('controllers_reward', False, True)
    eng, out = fused('policy_rows', True, False, agent_obs='all')
    w = torch.tensor(WEIGHTS, device='cuda:0')

    def unfused():
        eng.rollout(T, out=out, with_obs=False, logp=True, net_index=True, agent_obs='all')
        return torch_reward(torch, out['agent_obs'], eng.agent_observations('all'), out['reward'], w)
    arms['unfused'] = unfused
    names['unfused'] = eng.kernel_name() + ' + torch'
    torch.cuda.synchronize()
    return torch, arms, names


def bench_match(tree):
    """one `bench.py --task match --steps 16` in `tree`: the measure_match call behind secondary.match_8192"""
    r = subprocess.run([sys.executable, 'bench.py', '--task', 'match', '--gpus', '1', '--steps', '16', '--warmup', '4'], cwd=tree,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f'bench.py in {tree} failed:\n{r.stdout}\n{r.stderr}')
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return {'value': line['value'], 'repeats': line['repeats']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--launches', type=int, default=8)
    ap.add_argument('--warmup', type=float, default=1.0)
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    n, T = a.n, a.T
    res = {'n': n, 'T': T, 'noise': True, 'weights': WEIGHTS,
           'protocol': {'regions': a.regions, 'launches_per_region': a.launches, 'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    # the unchanged path first, before this process opens the device: parent and tree alternate, a process each
    if a.parent_tree:
        runs = {'parent': [], 'tree': []}
        for _ in range(a.bench_rounds):
            runs['parent'].append(bench_match(os.path.abspath(a.parent_tree)))
            runs['tree'].append(bench_match(ROOT))
        med = {k: sorted(r['value'] for r in v)[len(v) // 2] for k, v in runs.items()}
        res['match_8192'] = {'unit': 'env-steps/s', 'parent': med['parent'], 'tree': med['tree'], 'tree_over_parent': med['tree'] / med['parent'],
                             'within_5_percent': bool(abs(med['tree'] / med['parent'] - 1.0) <= 0.05), 'runs': runs,
                             'what': 'median of the runs; a run is bench.py --task match --gpus 1 --steps 16 --warmup 4 (its value: the median region)'}
    else:
        res['match_8192'] = 'not measured'
    torch, arms, names = arms_of(n, T)
    res['device'], res['kernel'] = torch.cuda.get_device_name(0), names

    def run(fn, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / count

    def warm(fn, seconds):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            run(fn, 1)
    times = {k: [] for k in arms}
    for k, fn in arms.items():
        warm(fn, a.warmup)
    for _ in range(a.regions):
        for k, fn in arms.items():
            warm(fn, 0.1)
            times[k].append(run(fn, a.launches))
    med = {}
    for k, v in times.items():
        s = sorted(v)
        med[k] = s[len(s) // 2]
        res[k] = {'seconds_per_T_cycles': {'median': med[k], 'min': s[0], 'max': s[-1], 'regions': v},
                  'match_steps_per_s': {'median': n * T / med[k], 'min': n * T / s[-1], 'max': n * T / s[0]}}
    res['policy_reward_over_policy_time'] = med['policy_reward'] / med['policy']
    res['controllers_reward_over_controllers_time'] = med['controllers_reward'] / med['controllers']
    res['unfused_over_policy_reward_time'] = med['unfused'] / med['policy_reward']
    res['policy_rows_over_policy_time'] = med['policy_rows'] / med['policy']
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
