"""The fused PPO minibatch step (soccer2d_amd.learn.PPOLearner: s2d_learn_ppo) against the chain of torch ops it replaces in
examples/ppo_reach_ball.py's DevicePPO.update and examples/ppo_match_selfplay.py's loop, in ONE process, both eagerly and replayed
from a captured graph.  A call is ONE minibatch step of B rows named by a permutation slice in a rollout of 2 B rows.

  reach_ball     pi 10-64-64-16, vf 10-64-64-1 Tanh, categorical      B = 32 768     the example at --envs 4096 --fused-actor 32 --tanh
  turning        pi 10-64-64-4, vf 10-64-64-1 ReLU, Gaussian          B = 32 768     --turning
  match_11v11    pi 224-64-64-16, vf 224-64-64-1 Tanh, categorical    B = 180 224    ppo_match_selfplay.py's defaults (1024 x 64 x 22 / 8)
  small_batch    as reach_ball                                        B = 4 096
  wide_256_256   pi 10-256-256-16, vf 10-256-256-1 Tanh, categorical  B = 32 768     the widest layers of the grid

The torch chain is the examples', gathers included: obs[i], act[i], adv[i], logp_old[i], ret[i]; two forwards; Categorical or Normal;
log_prob, entropy; the advantage normalisation; exp, min / clamp; mse_loss; zero_grad, backward, Adam.step -- eagerly with
torch.optim.Adam as the examples make it, under capture with Adam(capturable=True); the distributions are made with
validate_args=False in both torch arms (their checks synchronise, which a capture forbids).  The fused step is PPOLearner.step(rollout, index)
with the same Adam arguments and no gradient clip.  Protocol as in learn_rate.py: every arm warmed up for `--warmup` seconds of
back-to-back work, then `--regions` timed regions per arm, the arms alternating; a region is a number of calls (sized to about
`--region-seconds`) between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and the
highest, in seconds per call, and ratios of the medians (above 1: the fused step is faster).  Both learners start from the same
weights; after one step on the same minibatch the largest parameter difference is recorded (different summation orders and
elementary functions: not bitwise).

Prints one JSON object; profiles/r14/learn_ppo_rate.json holds a run.
    python profiles/experiments/learn_ppo_rate.py [--regions 5] [out.json]"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from soccer2d_amd.learn import PPOLearner  # noqa: E402

# (name, D, hidden, A, activation, Gaussian, B)
CONFIGS = (('reach_ball', 10, (64, 64), 16, nn.Tanh, False, 32768), ('turning', 10, (64, 64), 4, nn.ReLU, True, 32768),
           ('match_11v11', 224, (64, 64), 16, nn.Tanh, False, 180224), ('small_batch', 10, (64, 64), 16, nn.Tanh, False, 4096),
           ('wide_256_256', 10, (256, 256), 16, nn.Tanh, False, 32768))
CLIP, VF_COEF, ENT_COEF, LR = 0.2, 0.5, 0.01, 3e-4


def mlp(n_in, hidden, n_out, act):
    layers = []
    for w in hidden:
        layers += [nn.Linear(n_in, w), act()]
        n_in = w
    return nn.Sequential(*layers, nn.Linear(n_in, n_out))


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


def captured(fn):
    """fn as a graph replay: a warm-up on a side stream, then one capture"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    torch.cuda.synchronize()
    return graph.replay


class TorchPPO:
    """one minibatch step of the examples' loop"""

    def __init__(self, pi, vf, log_std, capturable):
        self.pi, self.vf, self.log_std = pi, vf, log_std
        params = list(pi.parameters()) + list(vf.parameters()) + ([log_std] if log_std is not None else [])
        self.opt = torch.optim.Adam(params, lr=LR, **(dict(capturable=True) if capturable else {}))

    def step(self, ro, i):
        y = self.pi(ro['obs'][i])
        if self.log_std is None:                          # validate_args=False: the checks synchronise, which a capture forbids
            d = torch.distributions.Categorical(logits=y, validate_args=False)
        else:
            d = torch.distributions.Independent(torch.distributions.Normal(y, self.log_std.exp().expand_as(y), validate_args=False), 1,
                                                validate_args=False)
        logp = d.log_prob(ro['action'][i])
        a = ro['advantage'][i]
        a = (a - a.mean()) / (a.std() + 1e-8)
        ratio = (logp - ro['logp'][i]).exp()
        pg = -torch.min(ratio * a, ratio.clamp(1 - CLIP, 1 + CLIP) * a).mean()
        v_loss = nn.functional.mse_loss(self.vf(ro['obs'][i]).squeeze(-1), ro['return'][i])
        loss = pg + VF_COEF * v_loss - ENT_COEF * d.entropy().mean()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()


def flat(pi, vf, log_std):
    return torch.cat([p.detach().reshape(-1) for m in (pi, vf) for p in m.parameters()] + ([log_std.detach().reshape(-1)] if log_std is not None else []))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--region-seconds', type=float, default=0.25)
    ap.add_argument('--warmup', type=float, default=0.5)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('learn_ppo_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    dev = 'cuda:0'
    res = {'device': torch.cuda.get_device_name(0), 'library': os.environ.get('S2D_LIB', 'this tree'),
           'hyper': {'lr': LR, 'clip_range': CLIP, 'vf_coef': VF_COEF, 'ent_coef': ENT_COEF, 'normalize_advantage': True, 'max_grad_norm': 0.0},
           'protocol': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup, 'arms': 'alternating',
                        'call': 'one minibatch step of B rows, a permutation slice of a rollout of 2 B rows'}}
    for name, D, hidden, A, act, gauss, B in CONFIGS:
        R = 2 * B
        pi0, vf0 = mlp(D, hidden, A, act).to(dev), mlp(D, hidden, 1, act).to(dev)
        ls0 = torch.full((A,), -0.5, device=dev) if gauss else None
        perm = torch.randperm(R, device=dev)[:B]
        i64, i32 = perm.contiguous(), perm.int().contiguous()
        with torch.no_grad():
            obs = torch.rand(R, D, device=dev) * 2 - 1
            y = pi0(obs)
            if gauss:
                dist = torch.distributions.Independent(torch.distributions.Normal(y, ls0.exp().expand_as(y)), 1)
            else:
                dist = torch.distributions.Categorical(logits=y)
            action = dist.sample()
            logp = dist.log_prob(action) + 0.1 * torch.randn(R, device=dev)   # a policy a few steps old: some ratios beyond the clip
            ret = vf0(obs).squeeze(-1) + torch.randn(R, device=dev)
        ro64 = {'obs': obs, 'action': action, 'logp': logp, 'advantage': torch.randn(R, device=dev), 'return': ret}
        ro32 = dict(ro64, action=action if gauss else action.int())

        def fresh():
            return copy.deepcopy(pi0), copy.deepcopy(vf0), (nn.Parameter(ls0.clone()) if gauss else None)

        def fused_of(mods):
            return PPOLearner.from_modules(*mods, lr=LR, eps=1e-8, max_grad_norm=0.0, clip_range=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF,
                                           max_batch=B)
        # one step of each from the same weights on the same minibatch
        ma, mb = fresh(), fresh()
        la = fused_of(ma)
        la.step(ro32, i32)
        TorchPPO(*mb, False).step(ro64, i64)
        torch.cuda.synchronize()
        entry = {'networks': 'pi ' + '-'.join(map(str, (D,) + hidden + (A,))) + ', vf ' + '-'.join(map(str, (D,) + hidden + (1,))) + ' ' + act.__name__ +
                 (', Gaussian' if gauss else ', categorical'), 'batch': B, 'rollout_rows': R, 'parameters': la.params.numel(),
                 'workspace_bytes': la.workspace.numel() * 4, 'clip_fraction_of_the_minibatch': la.clip_fraction,
                 'max_abs_parameter_difference_after_one_step': float((flat(*ma) - flat(*mb)).abs().max()),
                 'parameter_change_of_that_step': float((flat(*mb) - flat(pi0, vf0, ls0)).abs().max())}
        fused = [fused_of(fresh()) for _ in range(2)]
        tch = [TorchPPO(*fresh(), False), TorchPPO(*fresh(), True)]
        arms = [('fused_eager', lambda: fused[0].step(ro32, i32)), ('torch_eager', lambda: tch[0].step(ro64, i64)),
                ('fused_graph', captured(lambda: fused[1].step(ro32, i32))), ('torch_graph', captured(lambda: tch[1].step(ro64, i64)))]
        counts, times = {}, {n: [] for n, _ in arms}
        for n, fn in arms:
            warm(fn, a.warmup)
            counts[n] = max(5, int(a.region_seconds / region(fn, 5)))
        for _ in range(a.regions):
            for n, fn in arms:
                warm(fn, 0.05)                                 # back on this arm's code and clock after the other arms
                times[n].append(region(fn, counts[n]))
        med = {}
        for n, _ in arms:
            v = sorted(times[n])
            med[n] = v[len(v) // 2]
            entry[n] = {'seconds_per_call': {'median': med[n], 'min': v[0], 'max': v[-1], 'regions': times[n]}, 'calls_per_region': counts[n]}
        entry['torch_over_fused_eager'] = med['torch_eager'] / med['fused_eager']
        entry['torch_over_fused_graph'] = med['torch_graph'] / med['fused_graph']
        res[name] = entry
        print(name, {k: (v['seconds_per_call']['median'] if isinstance(v, dict) else v) for k, v in entry.items()}, file=sys.stderr, flush=True)
        del ro64, ro32, obs, fused, tch, arms
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
