"""The fused Q-learner step (soccer2d_amd.learn.QLearner: s2d_learn_q) against the chain of torch ops it replaces in
examples/dqn_reach_ball.py's optimise_fused, at B = 4096, in ONE process, both eagerly and replayed from a captured graph.

  relu_64_64       10-64-64-16 ReLU             SB3's default
  gtc_64_64        4-64-64-16 ReLU              the GoToCenter observation
  tanh_128_16      10-128-64-32-16-16 Tanh      the reference's net_arch
  wide_in_224      224-64-64-16 ReLU            the 11v11 agent row
  relu_256_256     10-256-256-16 ReLU

The torch chain is the example's: q(obs).gather, smooth_l1_loss, zero_grad, backward, clip_grad_norm_(10), Adam.step -- eagerly
with torch.optim.Adam as the example makes it, under capture with Adam(capturable=True).  Per configuration four arms (the fused
step and the torch chain, each eager and as a graph replay) and a fifth: the whole captured chain sample -> target -> step
(DeviceReplay.sample, QTarget.target, QLearner.step in one graph).  Protocol as in td_target_rate.py: every arm warmed up for
`--warmup` seconds of back-to-back work, then `--regions` timed regions per arm, the arms alternating; a region is a number of
calls (sized to about `--region-seconds`) between two host clocks that end in a device synchronise.  Reported per arm: the median
region, the lowest and the highest, in seconds per call, and ratios of the medians (above 1: the fused step is faster).  The
learners start from the same weights; after one step on the same batch the largest parameter difference is recorded (different
summation orders and Adam's bias correction in fp32: not bitwise).

Prints one JSON object; profiles/r12/learn_rate.json holds a run.
    python profiles/experiments/learn_rate.py [--batch 4096] [--regions 5] [out.json]"""
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

from soccer2d_amd.learn import QLearner  # noqa: E402
from soccer2d_amd.replay import DeviceReplay  # noqa: E402
from soccer2d_amd.td import QTarget  # noqa: E402

CONFIGS = (('relu_64_64', 10, (64, 64), nn.ReLU), ('gtc_64_64', 4, (64, 64), nn.ReLU), ('tanh_128_16', 10, (128, 64, 32, 16), nn.Tanh),
           ('wide_in_224', 224, (64, 64), nn.ReLU), ('relu_256_256', 10, (256, 256), nn.ReLU))
N_ACT = 16


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


def torch_chain(q, opt, b, tgt):
    """one update of examples/dqn_reach_ball.py's optimise_fused (the uniform-replay arm)"""
    def step():
        qa = q(b['obs']).gather(1, b['action'].long()).squeeze(1)
        loss = nn.functional.smooth_l1_loss(qa, tgt)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        nn.utils.clip_grad_norm_(q.parameters(), 10.0)
        opt.step()
    return step


def filled_replay(dev, D, B):
    """a DeviceReplay of obs_dim D holding one synthetic record of 8 x 1024 transitions"""
    T, N = 8, 1024
    rb = DeviceReplay(1 << 16, D, device=dev, seed=3)
    rec = {'obs': torch.randn(T, N, D, device=dev), 'terminal_obs': torch.randn(T, N, D, device=dev),
           'action': torch.randint(0, N_ACT, (T, N), dtype=torch.int32, device=dev), 'reward': torch.randn(T, N, device=dev),
           'done': (torch.rand(T, N, device=dev) < 0.05).to(torch.uint8)}
    rb.push(rec, torch.randn(N, D, device=dev))
    return rb, rb.alloc_batch(B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--region-seconds', type=float, default=0.25)
    ap.add_argument('--warmup', type=float, default=0.5)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('learn_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    dev, B = 'cuda:0', a.batch
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'library': os.environ.get('S2D_LIB', 'this tree'),
           'protocol': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    for name, D, hidden, act in CONFIGS:
        q0 = mlp(D, hidden, N_ACT, act).to(dev)
        b = {'obs': torch.randn(B, D, device=dev), 'action': torch.randint(0, N_ACT, (B, 1), dtype=torch.int32, device=dev)}
        tgt = torch.randn(B, device=dev)

        def fresh():
            return copy.deepcopy(q0)
        # one step of each from the same weights on the same batch
        qa, qb = fresh(), fresh()
        la = QLearner.from_module(qa, max_batch=B)
        la.step(b, tgt)
        torch_chain(qb, torch.optim.Adam(qb.parameters(), lr=1e-3), b, tgt)()
        torch.cuda.synchronize()
        flat = torch.cat([p.detach().reshape(-1) for p in qb.parameters()])
        entry = {'network': '-'.join(map(str, (D,) + hidden + (N_ACT,))) + ' ' + act.__name__, 'parameters': flat.numel(),
                 'max_abs_parameter_difference_after_one_step': float((la.params - flat).abs().max()),
                 'parameter_change_of_that_step': float((flat - torch.cat([p.detach().reshape(-1) for p in q0.parameters()])).abs().max())}
        # the arms, each on a learner of its own
        fused = [QLearner.from_module(fresh(), max_batch=B) for _ in range(2)]
        tq = [fresh() for _ in range(2)]
        opts = [torch.optim.Adam(tq[0].parameters(), lr=1e-3), torch.optim.Adam(tq[1].parameters(), lr=1e-3, capturable=True)]
        rb, batch = filled_replay(dev, D, B)
        chain_learner, chain_td, chain_tgt = QLearner.from_module(fresh(), max_batch=B), QTarget.from_module(fresh()), torch.empty(B, device=dev)

        def chain():
            chain_learner.step(rb.sample(B, out=batch), chain_td.target(batch, out=chain_tgt))
        arms = [('fused_eager', lambda: fused[0].step(b, tgt)), ('torch_eager', torch_chain(tq[0], opts[0], b, tgt)),
                ('fused_graph', captured(lambda: fused[1].step(b, tgt))), ('torch_graph', captured(torch_chain(tq[1], opts[1], b, tgt))),
                ('sample_target_step_graph', captured(chain))]
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
