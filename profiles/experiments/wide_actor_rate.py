"""Rate of the fused actors on the streamed-weight MLP (Engine.rollout_qnet / rollout_actor with the Wide* classes) against the
resident path where that exists and against the torch-in-the-loop step, in one process.  The protocol of mlp_actor_rate.py:
65 536 envs, eps = 0.05, full record + terminal observations, noise off; every arm is one captured graph (the pack kernel is in
it), timed `--repeats` times after a warm-up with the arms ALTERNATED (one replay of each per round); the figure is the median.
T is chosen so that a launch lasts a few ms: 256 for 10-64-64-16, 32 for the large shapes.

  a  rollout_qnet, MlpQNetActor 10-64-64-16 ReLU           the resident kernel
  b  rollout_qnet, WideQNetActor on the same network       b / a = the price of streaming where residency was possible
  c  rollout_actor, WideDeterministicActor [400, 300] ReLU, A = 1, Gaussian noise   the reference's default DDPG
  d  rollout_qnet, WideQNetActor [256, 256] ReLU
  e  rollout_qnet, WideQNetActor [400] * 5 Tanh
  f  rollout_qnet, WideQNetActor [400] * 5 Sigmoid
  c' d' e' f'  s2d_step with the same torch module in the loop (one graph of 16 steps)

Per wide shape also: the MFMAs per env-tile step (one per weight fragment) x 32 clocks = the matrix pipe's issue floor with one
wave on every SIMD (256 CUs x 4 SIMDs, at the clock read from the device, else 2.4 GHz), the achieved fraction of it, and the
weight bytes a wave fetches per env-step (fragments x 256 bytes per pass of 16 x tiles envs).

Usage: python profiles/experiments/wide_actor_rate.py [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'gym-soccer-2d-env_amd')):
    sys.path.insert(0, p)

import torch  # noqa: E402

from soccer2d_amd.engine import Engine, make_config  # noqa: E402
from soccer2d_amd.mlp_actor import MlpQNetActor  # noqa: E402
from soccer2d_amd.wide_actor import WideDeterministicActor, WideQNetActor, wide_plan  # noqa: E402

DQN = dict(change_ball_position=True, change_ball_velocity=True, min_distance_to_ball=5.0, max_steps=200,
           use_continuous_action=False, action_space_size=16, use_turning=False)
DDPG = dict(DQN, use_continuous_action=True)
N, LOOP_STEPS, SIMDS = 65536, 16, 256 * 4
ACT = {'relu': torch.nn.ReLU, 'tanh': torch.nn.Tanh, 'sigmoid': torch.nn.Sigmoid}


def module(hidden, act, na=16, tanh_head=False):
    torch.manual_seed(0)
    layers, win = [], 10
    for w in hidden:
        layers += [torch.nn.Linear(win, w), ACT[act]()]
        win = w
    layers.append(torch.nn.Linear(win, na))
    if tanh_head:
        layers.append(torch.nn.Tanh())
    return torch.nn.Sequential(*layers).to('cuda:0')


def capture(fn, launches, settle_s=1.0):
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


def fused_arm(actor, T, task=DQN, launches=2):
    eng = Engine(N, 'cuda:0', cfg=make_config(noise=False, **task))
    eng.reset()
    out = eng.alloc_rollout(T, terminal_obs=True)
    roll = eng.rollout_actor if task is DDPG else eng.rollout_qnet
    g = capture(lambda: roll(T, actor, out=out), launches)
    return dict(graph=g, launches=launches, steps=N * T, T=T, keep=(eng, actor, out), kernel=eng.kernel_name())


def loop_arm(net, task=DQN):
    eng = Engine(N, 'cuda:0', cfg=make_config(noise=False, **task))
    eng.reset()

    def one():
        with torch.no_grad():
            if task is DDPG:
                act = net(eng.obs)
                eng.step((act + 0.1 * torch.randn_like(act)).clamp(-1, 1))
            else:
                eng.step(net(eng.obs).argmax(dim=1))
    g = capture(one, LOOP_STEPS)
    return dict(graph=g, launches=LOOP_STEPS, steps=N, T=1, keep=(eng, net), kernel='s2d_step + torch fp32 forward')


def device_clock_hz():
    """the shader clock the device reports while busy (read only), or None"""
    try:
        txt = subprocess.run(['rocm-smi', '--showclocks'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=30).stdout
        mhz = [int(m) for m in re.findall(r'sclk clock level:[^\n]*\((\d+)Mhz\)', txt)]
        return max(mhz) * 1e6 if mhz else None
    except Exception:  # noqa: BLE001
        return None


def fragments(hidden, na):
    nfrag, ks = 0, 3
    for w in hidden:
        nfrag += (w + 15) // 16 * ks
        ks = w // 4
    return nfrag + (na + 15) // 16 * ks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    small = module((64, 64), 'relu')
    ddpg = module((400, 300), 'relu', 1, tanh_head=True)
    q256 = module((256, 256), 'relu')
    deep_t, deep_s = module((400,) * 5, 'tanh'), module((400,) * 5, 'sigmoid')
    shapes = {'b': ((64, 64), 16), 'c': ((400, 300), 1), 'd': ((256, 256), 16), 'e': ((400,) * 5, 16), 'f': ((400,) * 5, 16)}
    arms = {
        'a_mlp_10-64-64-16_relu': fused_arm(MlpQNetActor.from_module(small, epsilon=0.05), 256),
        'b_wide_10-64-64-16_relu': fused_arm(WideQNetActor.from_module(small, epsilon=0.05), 256),
        'c_wide_actor_10-400-300-1_relu_gauss': fused_arm(WideDeterministicActor.from_module(ddpg, epsilon=0.05, noise_sigma=0.1), 32,
                                                          task=DDPG),
        'c_torch_in_the_loop': loop_arm(ddpg, task=DDPG),
        'd_wide_10-256-256-16_relu': fused_arm(WideQNetActor.from_module(q256, epsilon=0.05), 32),
        'd_torch_in_the_loop': loop_arm(q256),
        'e_wide_10-400x5-16_tanh': fused_arm(WideQNetActor.from_module(deep_t, epsilon=0.05), 32, launches=1),
        'e_torch_in_the_loop': loop_arm(deep_t),
        'f_wide_10-400x5-16_sigmoid': fused_arm(WideQNetActor.from_module(deep_s, epsilon=0.05), 32, launches=1),
        'f_torch_in_the_loop': loop_arm(deep_s),
    }
    walls = {k: [] for k in arms}
    for _ in range(2):                                     # one untimed round of every arm behind the captures
        for arm in arms.values():
            arm['graph'].replay()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for k, arm in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); arm['graph'].replay(); e1.record(); e1.synchronize()
            walls[k].append(e0.elapsed_time(e1) * 1e-3 / arm['launches'])
    for _ in range(20):                                    # untimed: the clock the device grants while arm e runs
        arms['e_wide_10-400x5-16_tanh']['graph'].replay()
    clock = device_clock_hz()
    torch.cuda.synchronize()
    hz = clock or 2.4e9
    res = {'device': torch.cuda.get_device_name(0), 'envs': N, 'epsilon': 0.05, 'repeats': a.repeats,
           'shader_clock_hz': hz, 'shader_clock_source': 'rocm-smi --showclocks while arm e runs, after the timed rounds' if clock else 'nominal (not read)'}
    for k, arm in arms.items():
        w = sorted(walls[k])
        per = w[len(w) // 2]
        res[k] = {'T': arm['T'], 'us_per_launch': per * 1e6, 'env_steps_per_s': arm['steps'] / per, 'kernel': arm['kernel'],
                  'repeats_us': [v * 1e6 for v in w]}
        if k[0] in shapes and '_wide' in k:
            hidden, na = shapes[k[0]]
            waves, tiles, lds, ws = wide_plan(hidden, na)
            nfrag = fragments(hidden, na)
            floor_s = (N / 16) * nfrag * 32 / (SIMDS * hz) * arm['T']      # every SIMD issuing MFMAs back to back
            res[k].update({'waves': waves, 'tiles': tiles, 'lds_bytes': lds, 'workspace_bytes': ws, 'mfma_per_env_tile_step': nfrag,
                           'mfma_issue_clocks_per_env_tile_step': nfrag * 32, 'mfma_floor_us_per_launch': floor_s * 1e6,
                           'fraction_of_mfma_floor': floor_s / per, 'weight_bytes_per_env_step': nfrag * 256 / (16 * tiles)})
    rate = lambda k: res[k]['env_steps_per_s']  # noqa: E731
    res['b_over_a'] = rate('b_wide_10-64-64-16_relu') / rate('a_mlp_10-64-64-16_relu')
    for c, k in (('c', 'c_wide_actor_10-400-300-1_relu_gauss'), ('d', 'd_wide_10-256-256-16_relu'), ('e', 'e_wide_10-400x5-16_tanh'),
                 ('f', 'f_wide_10-400x5-16_sigmoid')):
        res[f'{c}_over_torch'] = rate(k) / rate(f'{c}_torch_in_the_loop')
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
