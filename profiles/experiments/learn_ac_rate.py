"""The fused DDPG update (soccer2d_amd.learn.ActorCriticLearner: s2d_learn_critic, s2d_learn_actor and update_targets) against the
chain of torch ops it replaces in examples/ddpg_reach_ball.py's optimise (the --fused-target arm), at B = 4096, in ONE process,
both eagerly and replayed from a captured graph.

  reach_ball       mu 10-64-64-1, q 11-64-64-1 ReLU                 the example's default
  turning          mu 10-64-64-4, q 14-64-64-1 ReLU                 --turning: the 4-D action
  ref_pi_qf        mu 10-16-8-1, q 11-64-32-16-8-1 ReLU             the reference's net_arch=dict(pi=[16, 8], qf=[64, 32, 16, 8])
  go_to_center     mu 4-16-8-4, q 8-64-32-16-8-1 ReLU               GoToCenter with --turn --useturn
  relu_256_256     mu 10-256-256-1, q 11-256-256-1 ReLU

The torch chain is the example's: q(cat(o, a)), mse_loss, zero_grad, backward, Adam.step; -q(cat(o, mu(o))).mean(), zero_grad,
backward, Adam.step; the Python loop of mul_ / add_ over every parameter tensor; ActorCriticTarget.sync() -- eagerly with
torch.optim.Adam as the example makes it, under capture with Adam(capturable=True).  The fused update is step_critic, step_actor and
update_targets(tau).  Per configuration seven arms: the whole update fused and in torch, each eager and as a graph replay, and the
fused update's three parts as graph replays of their own.  Protocol as in learn_rate.py: every arm warmed up for `--warmup` seconds
of back-to-back work, then `--regions` timed regions per arm, the arms alternating; a region is a number of calls (sized to about
`--region-seconds`) between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and
the highest, in seconds per call, and ratios of the medians (above 1: the fused update is faster).  Both learners start from the
same weights; after one update on the same batch the largest parameter difference is recorded (different summation orders: not
bitwise).

Prints one JSON object; profiles/r13/learn_ac_rate.json holds a run.
    python profiles/experiments/learn_ac_rate.py [--batch 4096] [--regions 5] [out.json]"""
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

from soccer2d_amd.learn import ActorCriticLearner  # noqa: E402
from soccer2d_amd.td import ActorCriticTarget  # noqa: E402

CONFIGS = (('reach_ball', 10, 1, (64, 64), (64, 64)), ('turning', 10, 4, (64, 64), (64, 64)), ('ref_pi_qf', 10, 1, (16, 8), (64, 32, 16, 8)),
           ('go_to_center', 4, 4, (16, 8), (64, 32, 16, 8)), ('relu_256_256', 10, 1, (256, 256), (256, 256)))
TAU = 0.005


def mlp(n_in, hidden, n_out, tanh=False):
    layers = []
    for w in hidden:
        layers += [nn.Linear(n_in, w), nn.ReLU()]
        n_in = w
    return nn.Sequential(*layers, nn.Linear(n_in, n_out), *([nn.Tanh()] if tanh else []))


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


class TorchDDPG:
    """one update of examples/ddpg_reach_ball.py's optimise after the target launch (the uniform-replay, --fused-target arm)"""

    def __init__(self, mu, q, capturable):
        self.mu, self.q = mu, q
        self.mu_target, self.q_target = copy.deepcopy(mu), copy.deepcopy(q)
        kw = dict(capturable=True) if capturable else {}
        self.opt_mu, self.opt_q = torch.optim.Adam(mu.parameters(), lr=1e-3, **kw), torch.optim.Adam(q.parameters(), lr=1e-3, **kw)
        self.td = ActorCriticTarget.from_modules(self.mu_target, self.q_target)

    def update(self, b, tgt):
        o, a = b['obs'], b['action']
        loss_q = nn.functional.mse_loss(self.q(torch.cat([o, a], 1)).squeeze(1), tgt)
        self.opt_q.zero_grad(set_to_none=True)
        loss_q.backward()
        self.opt_q.step()
        loss_mu = -self.q(torch.cat([o, self.mu(o)], 1)).mean()
        self.opt_mu.zero_grad(set_to_none=True)
        loss_mu.backward()
        self.opt_mu.step()
        with torch.no_grad():
            for net, tgt_net in ((self.mu, self.mu_target), (self.q, self.q_target)):
                for p, pt in zip(net.parameters(), tgt_net.parameters()):
                    pt.mul_(1 - TAU).add_(p, alpha=TAU)
        self.td.sync()


class FusedDDPG:
    def __init__(self, mu, q, B):
        self.lrn = ActorCriticLearner.from_modules(mu, q, max_batch=B)
        self.td = ActorCriticTarget.from_modules(copy.deepcopy(mu), copy.deepcopy(q))
        self.lrn.update_targets(self.td, TAU)                    # the mirrors exist before any capture

    def update(self, b, tgt):
        self.lrn.step_critic(b, tgt)
        self.lrn.step_actor(b)
        self.lrn.update_targets(self.td, TAU)


def flat(*mods):
    return torch.cat([p.detach().reshape(-1) for m in mods for p in m.parameters()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--region-seconds', type=float, default=0.25)
    ap.add_argument('--warmup', type=float, default=0.5)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('learn_ac_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    dev, B = 'cuda:0', a.batch
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'library': os.environ.get('S2D_LIB', 'this tree'), 'tau': TAU,
           'protocol': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    for name, D, A, ha, hc in CONFIGS:
        mu0, q0 = mlp(D, ha, A, tanh=True).to(dev), mlp(D + A, hc, 1).to(dev)
        b = {'obs': torch.randn(B, D, device=dev), 'action': torch.rand(B, A, device=dev) * 2 - 1}
        tgt = torch.randn(B, device=dev)

        def fresh():
            return copy.deepcopy(mu0), copy.deepcopy(q0)
        # one update of each from the same weights on the same batch
        ma, mb = fresh(), fresh()
        FusedDDPG(*ma, B).update(b, tgt)
        TorchDDPG(*mb, False).update(b, tgt)
        torch.cuda.synchronize()
        entry = {'networks': 'mu ' + '-'.join(map(str, (D,) + ha + (A,))) + ', q ' + '-'.join(map(str, (D + A,) + hc + (1,))) + ' ReLU',
                 'parameters': flat(mu0, q0).numel(),
                 'max_abs_parameter_difference_after_one_update': float((flat(*ma) - flat(*mb)).abs().max()),
                 'parameter_change_of_that_update': float((flat(*mb) - flat(mu0, q0)).abs().max())}
        fused = [FusedDDPG(*fresh(), B) for _ in range(3)]
        tch = [TorchDDPG(*fresh(), False), TorchDDPG(*fresh(), True)]
        parts = fused[2]
        arms = [('fused_eager', lambda: fused[0].update(b, tgt)), ('torch_eager', lambda: tch[0].update(b, tgt)),
                ('fused_graph', captured(lambda: fused[1].update(b, tgt))), ('torch_graph', captured(lambda: tch[1].update(b, tgt))),
                ('fused_critic_step_graph', captured(lambda: parts.lrn.step_critic(b, tgt))),
                ('fused_actor_step_graph', captured(lambda: parts.lrn.step_actor(b))),
                ('fused_update_targets_graph', captured(lambda: parts.lrn.update_targets(parts.td, TAU)))]
        counts, times = {}, {n: [] for n, _ in arms}
        for n, fn in arms:
            warm(fn, a.warmup)
            counts[n] = max(20, int(a.region_seconds / region(fn, 20)))
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
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
