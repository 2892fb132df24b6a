"""Rate of Soft Actor-Critic's two fused launches, in one process.

Collection, 65 536 envs x T = 256 steps, full record + terminal observations + logp, noise off, every arm one captured graph (the
pack kernel is in it), timed `--repeats` times after a warm-up with the arms ALTERNATED (wide_actor_rate.py's protocol; the
figure is the median).  Per hidden shape of [64, 64] and [256, 256] (ReLU, A = 1):
  sac     Engine.rollout_sac, SquashedGaussianActor 10-h-h-2
  actor   Engine.rollout_actor, WideDeterministicActor 10-h-h-1 with Gaussian action noise: the same launch without the
          state-dependent log-std, exp, log and logp
  torch   s2d_step with the torch module in the loop: Normal(mean, std).rsample(), tanh, log_prob with the tanh correction (one
          graph of 16 steps)

Target, B = 4096 (td_target_rate.py's protocol: alternating timed regions, each arm eager and as a graph replay), actor
10-h-h-2 and twin critics 11-h-h-1 for h = 64 and 256:
  launch  SacTarget.target
  torch   r + d * (min(q1', q2')(cat(s', a')) - alpha * logp) with a', logp sampled from the actor in torch

Prints one JSON object; profiles/r15/sac_rate.json holds a run.
    python profiles/experiments/sac_rate.py [--repeats 5] [--regions 5] [out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from soccer2d_amd.engine import Engine, make_config  # noqa: E402
from soccer2d_amd.td import SacTarget  # noqa: E402
from soccer2d_amd.wide_actor import SquashedGaussianActor, WideDeterministicActor  # noqa: E402

TASK = dict(change_ball_position=True, change_ball_velocity=True, min_distance_to_ball=5.0, max_steps=200,
            use_continuous_action=True, action_space_size=16, use_turning=False)
N, LOOP_STEPS, DEV = 65536, 16, 'cuda:0'


def mlp(n_in, hidden, n_out, tanh=False):
    layers = []
    for w in hidden:
        layers += [nn.Linear(n_in, w), nn.ReLU()]
        n_in = w
    layers.append(nn.Linear(n_in, n_out))
    return nn.Sequential(*(layers + ([nn.Tanh()] if tanh else []))).to(DEV)


def torch_sample(actor, obs):
    """SB3's squashed Gaussian: (a, logp)"""
    mean, log_std = actor(obs).chunk(2, dim=1)
    dist = torch.distributions.Normal(mean, log_std.clamp(-20.0, 2.0).exp(), validate_args=False)   # no host sync: capturable
    u = dist.rsample()
    a = torch.tanh(u)
    return a, (dist.log_prob(u) - torch.log(1 - a * a + 1e-6)).sum(dim=1)


# ------------------------------------------------------------------------------------------------------------------ collection
def capture(fn, launches, settle_s=0.5):
    t_end = time.perf_counter() + settle_s
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    g.replay(); torch.cuda.synchronize()
    return g


def fused_arm(actor, T, sac):
    eng = Engine(N, DEV, cfg=make_config(noise=False, **TASK))
    eng.reset()
    out = eng.alloc_rollout(T, terminal_obs=True, logp=sac)
    roll = eng.rollout_sac if sac else eng.rollout_actor
    g = capture(lambda: roll(T, actor, out=out), 1)
    return dict(graph=g, launches=1, steps=N * T, T=T, keep=(eng, actor, out), kernel=eng.kernel_name())


def loop_arm(actor):
    eng = Engine(N, DEV, cfg=make_config(noise=False, **TASK))
    eng.reset()

    def one():
        with torch.no_grad():
            eng.step(torch_sample(actor, eng.obs)[0])
    g = capture(one, LOOP_STEPS)
    return dict(graph=g, launches=LOOP_STEPS, steps=N, T=1, keep=(eng, actor), kernel='s2d_step + torch Normal / tanh / log_prob')


def collection(T, repeats):
    arms = {}
    for h in (64, 256):
        torch.manual_seed(h)
        pi = mlp(10, (h, h), 2)
        arms[f'sac_10-{h}-{h}-2'] = fused_arm(SquashedGaussianActor.from_module(pi, device=DEV), T, True)
        arms[f'actor_wide_gauss_10-{h}-{h}-1'] = fused_arm(
            WideDeterministicActor.from_module(mlp(10, (h, h), 1, tanh=True), device=DEV, epsilon=0.0, noise_sigma=0.1), T, False)
        arms[f'torch_in_the_loop_10-{h}-{h}-2'] = loop_arm(pi)
    walls = {k: [] for k in arms}
    for arm in arms.values():                              # one untimed round of every arm behind the captures
        arm['graph'].replay()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, arm in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); arm['graph'].replay(); e1.record(); e1.synchronize()
            walls[k].append(e0.elapsed_time(e1) * 1e-3 / arm['launches'])
    res = {}
    for k, arm in arms.items():
        w = sorted(walls[k])
        per = w[len(w) // 2]
        res[k] = {'T': arm['T'], 'us_per_launch': per * 1e6, 'env_steps_per_s': arm['steps'] / per, 'kernel': arm['kernel'],
                  'repeats_us': [v * 1e6 for v in w]}
    for h in (64, 256):
        sac = res[f'sac_10-{h}-{h}-2']['env_steps_per_s']
        res[f'sac_over_actor_wide_{h}'] = sac / res[f'actor_wide_gauss_10-{h}-{h}-1']['env_steps_per_s']
        res[f'sac_over_torch_in_the_loop_{h}'] = sac / res[f'torch_in_the_loop_10-{h}-{h}-2']['env_steps_per_s']
    return res


# ---------------------------------------------------------------------------------------------------------------------- target
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


def target(B, a):
    res = {}
    for h in (64, 256):
        torch.manual_seed(h)
        pi, q1, q2 = mlp(10, (h, h), 2), mlp(11, (h, h), 1), mlp(11, (h, h), 1)
        td = SacTarget(pi, q1, q2, seed=1, device=DEV)
        b = {'next_obs': torch.randn(B, 10, device=DEV), 'reward': torch.randn(B, device=DEV),
             'discount': torch.where(torch.rand(B, device=DEV) < 0.2, 0.0, 0.99).contiguous()}
        alpha, out = torch.tensor([0.2], device=DEV), torch.empty(B, device=DEV)

        def launch():
            return td.target(b, alpha, out=out)

        def chain():
            with torch.no_grad():
                n = b['next_obs']
                na, logp = torch_sample(pi, n)
                x = torch.cat([n, na], 1)
                return b['reward'] + b['discount'] * (torch.min(q1(x), q2(x)).squeeze(1) - alpha * logp)
        launch(); want = chain()
        torch.cuda.synchronize()
        # the two draw different noise: only the scale of the targets is comparable
        entry = {'mean_target_launch': float(out.mean()), 'mean_target_torch': float(want.mean())}
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
        res[f'target_{h}-{h}'] = entry
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=256, help='T of the collection launches')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--region-seconds', type=float, default=0.25)
    ap.add_argument('--warmup', type=float, default=0.5)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sac_rate.py measures on the GPU: no device found')
    res = {'device': torch.cuda.get_device_name(0), 'envs': N, 'batch': a.batch,
           'protocol': {'collection': {'repeats': a.repeats, 'arms': 'alternating graph replays, median'},
                        'target': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup,
                                   'arms': 'alternating'}}}
    res['collection'] = collection(a.steps, a.repeats)
    res['target'] = target(a.batch, a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
