"""11v11 self-play collection: the fused network rollout (MatchEngine.set_network + rollout) against the torch-in-the-loop cycle
(agent_observations -> torch MLP -> argmax -> gather from the action table -> rollout(1)), at 8192 matches, all 22 slots on one
224-64-64-16 network, T = 64 cycles per launch; the fused rollout with and without the left team's row record; and, to show
where the fused launch spends its time, the same launch without a network and the row-building kernel path without the forward
pass (all 22 rows built and recorded, no network).

Prints one JSON object (match-steps/s and agent decisions/s per variant); profiles/r05/match_net_rate.json holds a run.
    python profiles/experiments/match_net_rate.py [--n 8192] [--T 64] [--reps 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402

from soccer2d_amd.actor import MatchQNetActor  # noqa: E402
from soccer2d_amd.match import MatchEngine  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    n, T = a.n, a.T
    torch.manual_seed(0)
    q = torch.nn.Sequential(torch.nn.Linear(224, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                            torch.nn.Linear(64, 16)).cuda()
    g = torch.Generator().manual_seed(1)
    table = torch.stack([torch.randint(1, 5, (16,), generator=g).float(), torch.rand(16, generator=g) * 200 - 100,
                         torch.rand(16, generator=g) * 360 - 180], dim=1)
    actor = MatchQNetActor.from_module(q, table, epsilon=0.05)
    res = {'n': n, 'T': T, 'net': '224-64-64-16', 'slots': 22}

    eng = MatchEngine(n, 'cuda:0', noise=True)
    eng.set_network(actor)
    eng.reset()
    out = eng.alloc_rollout(T, with_obs=False)
    res['kernel'] = eng.kernel_name()
    for name, kw in (('fused', {}), ('fused_left_obs', {'agent_obs': 'left'})):
        s = timed(lambda: eng.rollout(T, out=out, with_obs=False, **kw), a.reps)
        res[name] = {'seconds_per_launch': s, 'match_steps_per_s': n * T / s, 'agent_decisions_per_s': 22 * n * T / s}
    eng.set_network(None)
    # where the time goes: the same engine with no network (the CTL kernel, every slot random), and the NET kernel building and
    # recording all 22 rows without a network (the rows' cost without the forward pass)
    eng.set_controllers([1] * 22)
    for name, kw in (('no_network', {}), ('rows_only', {'agent_obs': 'all'})):
        if 'agent_obs' in kw:
            out.pop('agent_obs', None)
        s = timed(lambda: eng.rollout(T, out=out, with_obs=False, **kw), a.reps)
        res[name] = {'seconds_per_launch': s, 'match_steps_per_s': n * T / s}
    eng.close()

    # the torch loop: one cycle per iteration, the same network and table, epsilon-greedy in torch
    eng = MatchEngine(n, 'cuda:0', noise=True)
    eng.reset()
    ro = eng.alloc_rollout(1, with_obs=False)
    obs = torch.empty((n, 22, 224), device='cuda:0')
    tab = table.cuda()

    def loop():
        with torch.no_grad():
            for _ in range(T):
                x = eng.agent_observations('all', out=obs)
                idx = q(x).argmax(dim=2)
                explore = torch.rand(idx.shape, device='cuda:0') < 0.05
                idx = torch.where(explore, torch.randint(0, 16, idx.shape, device='cuda:0'), idx)
                eng.rollout(1, actions=tab[idx].unsqueeze(0), out=ro, with_obs=False)
    s = timed(loop, a.reps)
    res['torch_loop'] = {'seconds_per_launch': s, 'match_steps_per_s': n * T / s, 'agent_decisions_per_s': 22 * n * T / s}
    res['speedup_fused_vs_torch'] = res['torch_loop']['seconds_per_launch'] / res['fused']['seconds_per_launch']
    eng.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
