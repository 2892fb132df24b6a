"""The TD-target launch (soccer2d_amd.td: s2d_td_target_q / s2d_td_target_ac) against the chain of torch ops it replaces in the
off-policy examples, at B = 4096, in ONE process, both eagerly and replayed from a captured graph.

  dqn          10-64-64-16        r + d * q_target(next).max(dim=1).values
  double_dqn   the same twice     r + d * q_target(next).gather(1, q(next).argmax(dim=1, keepdim=True)).squeeze(1)
  ddpg         actor 10-400-300-1 (Tanh head), critic 11-64-64-1     r + d * q_target(cat([next, mu_target(next)], 1)).squeeze(1)
  gtc_ddpg     the reference's pi: [16, 8] / qf: [64, 32, 16, 8] on GoToCenter's 4-word observation, the same chain
  dqn_224      224-64-64-16       the 11v11 agent row, the DQN chain

Per configuration four arms: the launch and the torch chain, each eager and as a graph replay (torch.cuda.graph).  Protocol as in
replay_prio_rate.py: every arm warmed up for `--warmup` seconds of back-to-back work, then `--regions` timed regions per arm, the
arms alternating; a region is a number of calls (sized to about `--region-seconds`) between two host clocks that end in a device
synchronise.  Reported per arm: the median region, the lowest and the highest, in seconds per call, and ratios of the medians.
The largest difference between the two results is recorded too (different summation orders: not bitwise).

Prints one JSON object; profiles/r11/td_target_rate.json holds a run.
    python profiles/experiments/td_target_rate.py [--batch 4096] [--regions 5] [out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from soccer2d_amd.td import ActorCriticTarget, QTarget  # noqa: E402


def mlp(n_in, hidden, n_out, tanh=False):
    layers = []
    for w in hidden:
        layers += [nn.Linear(n_in, w), nn.ReLU()]
        n_in = w
    layers.append(nn.Linear(n_in, n_out))
    return nn.Sequential(*(layers + ([nn.Tanh()] if tanh else [])))


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


def configurations(dev, B):
    """name -> (the launch writing `out`, the torch chain returning its result, out)"""
    def batch(D):
        return {'next_obs': torch.randn(B, D, device=dev), 'reward': torch.randn(B, device=dev),
                'discount': torch.where(torch.rand(B, device=dev) < 0.2, 0.0, 0.99).contiguous()}
    cfgs = {}

    def dqn(name, D, double):
        q_target, q = mlp(D, (64, 64), 16).to(dev), mlp(D, (64, 64), 16).to(dev)
        td, b, out = QTarget.from_module(q_target, online=q if double else None), batch(D), torch.empty(B, device=dev)
        if double:
            def chain():
                with torch.no_grad():
                    n = b['next_obs']
                    return b['reward'] + b['discount'] * q_target(n).gather(1, q(n).argmax(dim=1, keepdim=True)).squeeze(1)
        else:
            def chain():
                with torch.no_grad():
                    return b['reward'] + b['discount'] * q_target(b['next_obs']).max(dim=1).values
        cfgs[name] = (lambda: td.target(b, out=out), chain, out)

    def ddpg(name, D, A, pi, qf):
        mu_target, q_target = mlp(D, pi, A, tanh=True).to(dev), mlp(D + A, qf, 1).to(dev)
        td, b, out = ActorCriticTarget.from_modules(mu_target, q_target), batch(D), torch.empty(B, device=dev)

        def chain():
            with torch.no_grad():
                n = b['next_obs']
                return b['reward'] + b['discount'] * q_target(torch.cat([n, mu_target(n)], 1)).squeeze(1)
        cfgs[name] = (lambda: td.target(b, out=out), chain, out)

    dqn('dqn', 10, False)
    dqn('double_dqn', 10, True)
    ddpg('ddpg', 10, 1, (400, 300), (64, 64))
    ddpg('gtc_ddpg', 4, 1, (16, 8), (64, 32, 16, 8))
    dqn('dqn_224', 224, False)
    return cfgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--region-seconds', type=float, default=0.25)
    ap.add_argument('--warmup', type=float, default=0.5)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('td_target_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    dev, B = 'cuda:0', a.batch
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'library': os.environ.get('S2D_LIB', 'this tree'),
           'protocol': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    for name, (launch, chain, out) in configurations(dev, B).items():
        launch()
        want = chain()
        torch.cuda.synchronize()
        entry = {'max_abs_difference_launch_vs_torch': float((out - want).abs().max()), 'largest_abs_target': float(want.abs().max())}
        arms = [('launch_eager', launch), ('torch_eager', chain), ('launch_graph', captured(launch)), ('torch_graph', captured(chain))]
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
        entry['speedup_eager'] = med['torch_eager'] / med['launch_eager']
        entry['speedup_graph'] = med['torch_graph'] / med['launch_graph']
        res[name] = entry
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
