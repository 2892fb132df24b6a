"""The device replay buffer (soccer2d_amd.replay.DeviceReplay: s2d_replay_push / s2d_replay_sample) against the torch formulation
it replaces in the examples' learn_fused: 65 536 envs x T = 64, D = 10, a real rollout_qnet record with terminal observations, in
ONE process.

  push    DeviceReplay.push with n_step 1 and 3 (one copy launch + the cursor launch) against the chain the parent commit's
          learn_fused ran per record: cat to shift the observations, where over two [T,N,10] tensors, the term mask, five reshapes
          and five index scatters through an arange % cap index (1-step transitions only: torch has no n-step arm).
  sample  DeviceReplay.sample(B = 4096) against torch.randint + five gathers.

Protocol: every arm is warmed up for `--warmup` seconds of back-to-back work (past the clock ramp that follows an idle gap), then
`--regions` timed regions per arm, the arms alternating; a region is `--calls` calls between two host clocks that end in a
device synchronise.  Reported per arm: the median region, the lowest and the highest, in seconds per call; ratios of the medians;
and the bytes a transition holds over the push time.  The 1-step ring is compared bitwise with the torch buffer at the end.

Prints one JSON object; profiles/r09/replay_rate.json holds a run.
    python profiles/experiments/replay_rate.py [--n 65536] [--T 64] [--regions 5] [out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402

from soccer2d_amd.actor import QNetActor  # noqa: E402
from soccer2d_amd.engine import Engine, make_config  # noqa: E402
from soccer2d_amd.replay import DeviceReplay  # noqa: E402

TASK = dict(change_ball_position=True, change_ball_velocity=True, min_distance_to_ball=5.0, max_steps=200, action_space_size=16,
            use_continuous_action=False, use_turning=False)
GAMMA = 0.99


class TorchReplay:
    """the examples' replay buffer before DeviceReplay (dqn_reach_ball.py of the parent commit)"""

    def __init__(self, capacity, n_obs, device):
        self.cap, self.pos, self.full = capacity, 0, False
        self.obs = torch.empty((capacity, n_obs), device=device)
        self.next_obs = torch.empty((capacity, n_obs), device=device)
        self.act = torch.empty((capacity,), dtype=torch.int64, device=device)
        self.rew = torch.empty((capacity,), device=device)
        self.term = torch.empty((capacity,), device=device)

    def add(self, obs, act, rew, next_obs, term):
        n = obs.shape[0]
        idx = (torch.arange(n, device=obs.device) + self.pos) % self.cap
        self.obs[idx], self.act[idx], self.rew[idx], self.next_obs[idx], self.term[idx] = obs, act, rew, next_obs, term
        self.full |= self.pos + n >= self.cap
        self.pos = (self.pos + n) % self.cap

    def sample(self, batch):
        hi = self.cap if self.full else self.pos
        i = torch.randint(0, hi, (batch,), device=self.obs.device)
        return self.obs[i], self.act[i], self.rew[i], self.next_obs[i], self.term[i]


def torch_push(rb, rec, obs0):
    """learn_fused of the parent commit, from the rollout's return to rb.add"""
    obs_t = torch.cat([obs0[None], rec['obs'][:-1]])       # action t was chosen from the observation of step t - 1
    done = rec['done'].bool()
    next_obs = torch.where(done.unsqueeze(-1), rec['terminal_obs'], rec['obs'])   # bootstrap through Timeouts
    term = ((rec['result'] == 1) | (rec['result'] == 2)).float()                 # Goal / Out are true terminations
    rb.add(obs_t.reshape(-1, obs_t.shape[-1]), rec['action'].reshape(-1).long(), rec['reward'].reshape(-1),
           next_obs.reshape(-1, next_obs.shape[-1]), term.reshape(-1))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--capacity', type=int, default=1 << 23)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20, help='push calls per region')
    ap.add_argument('--sample-calls', type=int, default=2000)
    ap.add_argument('--warmup', type=float, default=1.0)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    n, T, B, cap = a.n, a.T, a.batch, max(a.capacity, a.n * a.T)
    if not torch.cuda.is_available():
        raise SystemExit('replay_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    dev = 'cuda:0'
    eng = Engine(n, dev, cfg=make_config(noise=True, **TASK))
    eng.reset()
    net = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 16)).cuda()
    actor = QNetActor.from_module(net, epsilon=0.3)
    eng.rollout_qnet(200, actor, with_obs=False)            # into the steady mix of episode ages
    obs0 = eng.obs.clone()
    rec = eng.rollout_qnet(T, actor, terminal_obs=True)
    torch.cuda.synchronize()
    D = rec['obs'].shape[-1]

    rb1 = DeviceReplay(cap, D, 1, torch.int32, dev, n_step=1, gamma=GAMMA)
    rb3 = DeviceReplay(cap, D, 1, torch.int32, dev, n_step=3, gamma=GAMMA)
    trb = TorchReplay(cap, D, dev)
    batch = rb1.alloc_batch(B)
    arms = [('push_n_step_1', lambda: rb1.push(rec, obs0), a.calls), ('push_n_step_3', lambda: rb3.push(rec, obs0), a.calls),
            ('torch_push', lambda: torch_push(trb, rec, obs0), a.calls),
            ('sample', lambda: rb1.sample(B, out=batch), a.sample_calls), ('torch_sample', lambda: trb.sample(B), a.sample_calls)]

    res = {'device': torch.cuda.get_device_name(0), 'n': n, 'T': T, 'obs_dim': D, 'batch': B, 'capacity': cap,
           'done_share': float(rec['done'].float().mean()), 'library': os.environ.get('S2D_LIB', 'this tree'),
           'protocol': {'regions': a.regions, 'push_calls_per_region': a.calls, 'sample_calls_per_region': a.sample_calls,
                        'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    times = {name: [] for name, _, _ in arms}
    for name, fn, _ in arms:
        warm(fn, a.warmup)
    for _ in range(a.regions):
        for name, fn, count in arms:
            warm(fn, 0.1)                                  # back on this arm's code and clock after the other arms
            times[name].append(region(fn, count))
    med = {}
    for name, _, _ in arms:
        v = sorted(times[name])
        med[name] = v[len(v) // 2]
        res[name] = {'seconds_per_call': {'median': med[name], 'min': v[0], 'max': v[-1], 'regions': times[name]}}
    moved = n * T * (4 * D * 4 + 4 + 4 + 1 + 1 + 4 + 4)     # obs_t + next read and written, action, reward, done, result, R, discount
    for k in ('push_n_step_1', 'push_n_step_3'):
        res[k]['transitions_per_s'] = n * T / med[k]
        res[k]['bytes_per_s_of_the_least_traffic'] = moved / med[k]
    res['speedup_push_n_step_1_vs_torch_push'] = med['torch_push'] / med['push_n_step_1']
    res['speedup_push_n_step_3_vs_torch_push_1_step'] = med['torch_push'] / med['push_n_step_3']
    res['speedup_sample_vs_torch_sample'] = med['torch_sample'] / med['sample']

    # the same transitions: one 1-step push into an empty ring against one torch add at position 0
    rb1.clear()
    rb1.push(rec, obs0)
    trb.pos, trb.full = 0, False
    torch_push(trb, rec, obs0)
    torch.cuda.synchronize()
    k = n * T
    w = lambda t: t.view(torch.int32)                      # noqa: E731
    res['one_step_ring_equals_torch_buffer_bitwise'] = bool(
        torch.equal(w(rb1.obs[:k]), w(trb.obs[:k])) and torch.equal(w(rb1.next_obs[:k]), w(trb.next_obs[:k])) and
        torch.equal(rb1.action[:k, 0].long(), trb.act[:k]) and torch.equal(w(rb1.reward[:k]), w(trb.rew[:k])) and
        torch.equal(w(rb1.discount[:k]), w((GAMMA * (1 - trb.term[:k])).contiguous())))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
