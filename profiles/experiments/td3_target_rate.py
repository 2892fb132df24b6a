"""TD3's target launch (soccer2d_amd.td.Td3Target: s2d_td_target_td3) against (a) the unsmoothed launch on the same shapes
(ActorCriticTarget: s2d_td_target_ac) -- the difference is the cost of the smoothing noise: one or two Philox blocks, two Box-Muller
pairs each, and the draws kernel behind the target kernel -- and (b) the chain of torch ops of examples/td3_reach_ball.py, at
B = 4096, in ONE process, both eagerly and replayed from a captured graph.

  reach_ball   actor 10-64-64-1 (Tanh head), critics 11-64-64-1 twice
  turning      actor 10-64-64-4, critics 14-64-64-1 twice: the 4-D action
  gtc          pi [16, 8] / qf [64, 32, 16, 8] on GoToCenter's 4-word observation, A = 1, twice
  sb3_default  actor 10-400-300-1, critics 11-64-64-1 twice

    torch chain:  a = mu'(n);  a' = (a + (sigma * randn_like(a)).clamp(-c, c)).clamp(-1, 1);  x = cat([n, a'], 1)
                  r + d * min(q1'(x), q2'(x)).squeeze(1)

Per configuration six arms: the TD3 launch, the unsmoothed launch and the torch chain, each eager and as a graph replay
(torch.cuda.graph).  Protocol as in td_target_rate.py: every arm warmed up for `--warmup` seconds of back-to-back work (the clock
ramp), then `--regions` timed regions per arm, the arms alternating; a region is a number of calls (sized to about
`--region-seconds`) between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and
the highest, in seconds per call; the noise's cost (TD3 launch - unsmoothed launch) and the ratios of the medians; and the shader
clock the device reports while the arms run (read only; null where it cannot be read).  With sigma = 0 the TD3 launch must give
the unsmoothed launch's targets: the largest difference is recorded and must be 0.

Prints one JSON object; profiles/r17/td3_target_rate.json holds a run.
    python profiles/experiments/td3_target_rate.py [--batch 4096] [--regions 5] [out.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from soccer2d_amd.td import ActorCriticTarget, Td3Target  # noqa: E402

SIGMA, CLIP = 0.2, 0.5


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


def busy_clock_mhz(fn, count):
    """the shader clock the device reports with `count` calls of fn in flight (read only), or None"""
    for _ in range(count):
        fn()
    try:
        txt = subprocess.run(['rocm-smi', '--showclocks'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=30).stdout
        mhz = [int(m) for m in re.findall(r'sclk clock level:[^\n]*\((\d+)Mhz\)', txt)]
    except Exception:  # noqa: BLE001
        mhz = []
    torch.cuda.synchronize()
    return max(mhz) if mhz else None


def configurations(dev, B):
    """name -> (the TD3 launch, the unsmoothed launch, the torch chain, the two launches' outputs, the Td3Target)"""
    cfgs = {}

    def add(name, D, A, pi, qf):
        mu, q1, q2 = mlp(D, pi, A, tanh=True).to(dev), mlp(D + A, qf, 1).to(dev), mlp(D + A, qf, 1).to(dev)
        b = {'next_obs': torch.randn(B, D, device=dev), 'reward': torch.randn(B, device=dev),
             'discount': torch.where(torch.rand(B, device=dev) < 0.2, 0.0, 0.99).contiguous()}
        td3, ac = Td3Target.from_modules(mu, q1, q2, target_policy_noise=SIGMA, target_noise_clip=CLIP, seed=1), ActorCriticTarget.from_modules(mu, q1, q2)
        out3, outa = torch.empty(B, device=dev), torch.empty(B, device=dev)

        def chain():
            with torch.no_grad():
                n = b['next_obs']
                a = mu(n)
                x = torch.cat([n, (a + (SIGMA * torch.randn_like(a)).clamp(-CLIP, CLIP)).clamp(-1, 1)], 1)
                return b['reward'] + b['discount'] * torch.min(q1(x), q2(x)).squeeze(1)
        cfgs[name] = (lambda: td3.target(b, out=out3), lambda: ac.target(b, out=outa), chain, out3, outa, td3)

    add('reach_ball', 10, 1, (64, 64), (64, 64))
    add('turning', 10, 4, (64, 64), (64, 64))
    add('gtc', 4, 1, (16, 8), (64, 32, 16, 8))
    add('sb3_default', 10, 1, (400, 300), (64, 64))
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
        raise SystemExit('td3_target_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    dev, B = 'cuda:0', a.batch
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'library': os.environ.get('S2D_LIB', 'this tree'), 'sigma': SIGMA, 'clip': CLIP,
           'protocol': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    for name, (td3, ac, chain, out3, outa, target) in configurations(dev, B).items():
        target.set_noise(0.0, CLIP)
        td3(), ac()
        torch.cuda.synchronize()
        entry = {'max_abs_difference_td3_sigma0_vs_unsmoothed': float((out3 - outa).abs().max())}
        if entry['max_abs_difference_td3_sigma0_vs_unsmoothed'] != 0.0:
            raise SystemExit(f'{name}: the TD3 launch at sigma = 0 differs from the unsmoothed launch')
        target.set_noise(SIGMA, CLIP)
        td3()
        want = chain()
        torch.cuda.synchronize()
        entry['mean_target_td3'], entry['mean_target_torch'] = float(out3.mean()), float(want.mean())    # other noise: the means only
        arms = [('td3_eager', td3), ('unsmoothed_eager', ac), ('torch_eager', chain), ('td3_graph', captured(td3)),
                ('unsmoothed_graph', captured(ac)), ('torch_graph', captured(chain))]
        counts, times = {}, {n: [] for n, _ in arms}
        for n, fn in arms:
            warm(fn, a.warmup)
            counts[n] = max(20, int(a.region_seconds / region(fn, 20)))
        entry['sclk_mhz_while_busy'] = busy_clock_mhz(arms[3][1], 20 * counts['td3_graph'])
        for _ in range(a.regions):
            for n, fn in arms:
                warm(fn, 0.05)                                 # back on this arm's code and clock after the other arms
                times[n].append(region(fn, counts[n]))
        med = {}
        for n, _ in arms:
            v = sorted(times[n])
            med[n] = v[len(v) // 2]
            entry[n] = {'seconds_per_call': {'median': med[n], 'min': v[0], 'max': v[-1], 'regions': times[n]}, 'calls_per_region': counts[n]}
        for kind in ('eager', 'graph'):
            entry[f'noise_cost_seconds_{kind}'] = med[f'td3_{kind}'] - med[f'unsmoothed_{kind}']
            entry[f'td3_over_unsmoothed_{kind}'] = med[f'td3_{kind}'] / med[f'unsmoothed_{kind}']
            entry[f'speedup_over_torch_{kind}'] = med[f'torch_{kind}'] / med[f'td3_{kind}']
        res[name] = entry
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
