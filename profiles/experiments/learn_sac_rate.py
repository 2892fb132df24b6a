"""The fused SAC update (soccer2d_amd.learn.SACLearner: s2d_learn_critic per critic, s2d_learn_sac_actor with the temperature, and
update_targets) against the chain of torch ops it replaces in examples/sac_reach_ball.py's optimise (the --fused-target arm), at
B = 4096, in ONE process, both eagerly and replayed from a captured graph.

  reach_ball       actor 10-64-64-2, q1 = q2 11-64-64-1 ReLU          the example's default
  turning          actor 10-64-64-8, q1 = q2 14-64-64-1 ReLU          --turning: the 4-D action
  relu_256_256     actor 10-256-256-2, q1 = q2 11-256-256-1 ReLU      SB3's default net_arch, three times: the image is in the workspace

The torch chain is the example's: 0.5 * (mse_loss(q1) + mse_loss(q2)), zero_grad, backward, Adam.step over both critics; the
reparameterised sample, (alpha * logp - min(q1, q2)).mean(), zero_grad, backward, Adam.step; the temperature's loss, backward,
Adam.step and alpha.copy_(exp); the Python loop of mul_ / add_ over every critic parameter; SacTarget.sync() -- eagerly with
torch.optim.Adam as the example makes it, under capture with Adam(capturable=True).  The fused update is step_critic, step_actor and
update_targets(tau).  Per configuration nine arms: the update fused and in torch, each eager and as a graph replay; the fused
update's three parts as graph replays of their own; and the WHOLE captured iteration, DeviceReplay.sample -> SacTarget.target ->
update, fused and in torch.  Protocol as in learn_ac_rate.py: every arm warmed up for `--warmup` seconds of back-to-back work (the
clock ramp), then `--regions` timed regions per arm, the arms alternating; a region is a number of calls (sized to about
`--region-seconds`) between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and
the highest, in seconds per call, and ratios of the medians (above 1: the fused update is faster).  Both learners start from the
same weights; their noise differs (Philox in the kernel, torch.randn in the chain), so after one update only the critics'
parameters are compared (different summation orders: not bitwise).

Prints one JSON object; profiles/r16/learn_sac_rate.json holds a run.
    python profiles/experiments/learn_sac_rate.py [--batch 4096] [--regions 5] [out.json]"""
import argparse
import copy
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from soccer2d_amd.learn import SACLearner  # noqa: E402
from soccer2d_amd.replay import DeviceReplay  # noqa: E402
from soccer2d_amd.td import SacTarget  # noqa: E402

CONFIGS = (('reach_ball', 10, 1, (64, 64), (64, 64)), ('turning', 10, 4, (64, 64), (64, 64)), ('relu_256_256', 10, 1, (256, 256), (256, 256)))
TAU = 0.005


def mlp(n_in, hidden, n_out):
    layers = []
    for w in hidden:
        layers += [nn.Linear(n_in, w), nn.ReLU()]
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


class TorchSAC:
    """one update of examples/sac_reach_ball.py's optimise after the target launch (the --fused-target arm)"""

    def __init__(self, actor, q1, q2, A, capturable):
        self.actor, self.q1, self.q2 = actor, q1, q2
        self.q1_target, self.q2_target = copy.deepcopy(q1), copy.deepcopy(q2)
        dev = next(actor.parameters()).device
        self.log_alpha = torch.zeros(1, device=dev, requires_grad=True)
        self.alpha = torch.ones(1, device=dev)
        self.target_entropy = -float(A)
        kw = dict(capturable=True) if capturable else {}
        self.opt_pi = torch.optim.Adam(actor.parameters(), lr=3e-4, **kw)
        self.opt_q = torch.optim.Adam(list(q1.parameters()) + list(q2.parameters()), lr=3e-4, **kw)
        self.opt_alpha = torch.optim.Adam([self.log_alpha], lr=3e-4, **kw)
        self.td = SacTarget.from_modules(actor, self.q1_target, self.q2_target)

    def sample_action(self, obs):
        mean, log_std = self.actor(obs).chunk(2, dim=1)
        log_std = log_std.clamp(-20.0, 2.0)
        z = torch.randn_like(mean)
        a = torch.tanh(mean + log_std.exp() * z)
        logp = (-0.5 * z * z - log_std - 0.5 * math.log(2 * math.pi) - torch.log(1 - a * a + 1e-6)).sum(dim=1)
        return a, logp

    def update(self, b, tgt):
        o, a = b['obs'], b['action']
        x = torch.cat([o, a], 1)
        loss_q = 0.5 * (nn.functional.mse_loss(self.q1(x).squeeze(1), tgt) + nn.functional.mse_loss(self.q2(x).squeeze(1), tgt))
        self.opt_q.zero_grad(set_to_none=True)
        loss_q.backward()
        self.opt_q.step()
        a_pi, logp = self.sample_action(o)
        x = torch.cat([o, a_pi], 1)
        loss_pi = (self.alpha * logp - torch.min(self.q1(x), self.q2(x)).squeeze(1)).mean()
        self.opt_pi.zero_grad(set_to_none=True)
        loss_pi.backward()
        self.opt_pi.step()
        loss_alpha = -(self.log_alpha * (logp.detach() + self.target_entropy).mean())
        self.opt_alpha.zero_grad(set_to_none=True)
        loss_alpha.backward()
        self.opt_alpha.step()
        with torch.no_grad():
            self.alpha.copy_(self.log_alpha.exp())
            for net, tgt_net in ((self.q1, self.q1_target), (self.q2, self.q2_target)):
                for p, pt in zip(net.parameters(), tgt_net.parameters()):
                    pt.mul_(1 - TAU).add_(p, alpha=TAU)
        self.td.sync()


class FusedSAC:
    def __init__(self, actor, q1, q2, B):
        self.lrn = SACLearner.from_modules(actor, q1, q2, max_batch=B)
        self.alpha = self.lrn.alpha
        self.td = SacTarget.from_modules(actor, copy.deepcopy(q1), copy.deepcopy(q2))
        self.lrn.update_targets(self.td, TAU)                    # the mirrors exist before any capture

    def update(self, b, tgt):
        self.lrn.step_critic(b, tgt)
        self.lrn.step_actor(b)
        self.lrn.update_targets(self.td, TAU)


class Loop:
    """the whole iteration on a replay buffer of its own: sample -> SacTarget.target -> update"""

    def __init__(self, model, rb, B):
        self.model, self.rb = model, rb
        self.batch, self.tgt = rb.alloc_batch(B), torch.empty(B, device=rb.device)

    def __call__(self):
        self.rb.sample(self.batch['obs'].shape[0], out=self.batch)
        self.model.td.target(self.batch, self.model.alpha, out=self.tgt)
        self.model.update(self.batch, self.tgt)


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
        raise SystemExit('learn_sac_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    dev, B = 'cuda:0', a.batch
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'library': os.environ.get('S2D_LIB', 'this tree'), 'tau': TAU,
           'protocol': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    for name, D, A, ha, hc in CONFIGS:
        mods0 = (mlp(D, ha, 2 * A).to(dev), mlp(D + A, hc, 1).to(dev), mlp(D + A, hc, 1).to(dev))
        b = {'obs': torch.randn(B, D, device=dev), 'action': torch.rand(B, A, device=dev) * 2 - 1}
        tgt = torch.randn(B, device=dev)
        T, N = 8, 2048
        rec = {'obs': torch.randn(T, N, D, device=dev), 'terminal_obs': torch.randn(T, N, D, device=dev),
               'action': torch.rand(T, N, A, device=dev) * 2 - 1, 'reward': torch.randn(T, N, device=dev),
               'done': (torch.rand(T, N, device=dev) < 0.05).to(torch.uint8)}

        def fresh():
            return tuple(copy.deepcopy(m) for m in mods0)

        def buffer():
            rb = DeviceReplay(T * N, D, action_words=A, action_dtype=torch.float32, device=dev, seed=1)
            rb.push(rec, torch.randn(N, D, device=dev))
            return rb
        # one update of each from the same weights on the same batch: the critics' steps see the same inputs
        ma, mb = fresh(), fresh()
        FusedSAC(*ma, B).update(b, tgt)
        TorchSAC(*mb, A, False).update(b, tgt)
        torch.cuda.synchronize()
        entry = {'networks': 'actor ' + '-'.join(map(str, (D,) + ha + (2 * A,))) + ', q1 = q2 ' + '-'.join(map(str, (D + A,) + hc + (1,))) + ' ReLU',
                 'parameters': flat(*mods0).numel(),
                 'max_abs_critic_parameter_difference_after_one_update': float((flat(*ma[1:]) - flat(*mb[1:])).abs().max()),
                 'critic_parameter_change_of_that_update': float((flat(*mb[1:]) - flat(*mods0[1:])).abs().max())}
        fused = [FusedSAC(*fresh(), B) for _ in range(4)]
        tch = [TorchSAC(*fresh(), A, False), TorchSAC(*fresh(), A, True), TorchSAC(*fresh(), A, True)]
        parts = fused[2]
        arms = [('fused_eager', lambda: fused[0].update(b, tgt)), ('torch_eager', lambda: tch[0].update(b, tgt)),
                ('fused_graph', captured(lambda: fused[1].update(b, tgt))), ('torch_graph', captured(lambda: tch[1].update(b, tgt))),
                ('fused_critic_step_graph', captured(lambda: parts.lrn.step_critic(b, tgt))),
                ('fused_actor_step_graph', captured(lambda: parts.lrn.step_actor(b))),
                ('fused_update_targets_graph', captured(lambda: parts.lrn.update_targets(parts.td, TAU))),
                ('fused_sample_target_update_graph', captured(Loop(fused[3], buffer(), B))),
                ('torch_sample_target_update_graph', captured(Loop(tch[2], buffer(), B)))]
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
        entry['torch_over_fused_whole_iteration_graph'] = med['torch_sample_target_update_graph'] / med['fused_sample_target_update_graph']
        res[name] = entry
        print(name, {k: (v['seconds_per_call']['median'] if isinstance(v, dict) else v) for k, v in entry.items()}, file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
