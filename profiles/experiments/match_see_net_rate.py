"""11v11 self-play collection under partial observability: the fused see-network rollout (MatchEngine.set_network with a see
actor + rollout: see rows, the 192-64-64-16 network, the body cycle and the vision step of all 22 players in one launch of T = 64
cycles) against the unfused cycle in the same process (see('all') -> the same torch module -> argmax -> gather from the action
table -> rollout(1) -> vision_step), at 8192 matches, all 22 slots on the network, epsilon 0.1, noise on; the fused rollout with
and without the see record of all 22 slots; and, to show where the fused launch spends its time, the same launch without a
network (the random policy, the vision state stepped in the kernel) with all 22 see rows built and recorded.

Protocol: every arm is warmed up for `--warmup` seconds of back-to-back work (past the clock ramp that follows an idle gap), then
`--regions` timed regions per arm, the arms alternating; a region is `--launches` fused launches (or `--loops` unfused loops of T
cycles) between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and the
highest, as seconds per T cycles, match-steps/s and agent decisions/s; and the ratio of the medians.  The shader clock is sampled
with `rocm-smi --showclocks` while the fused arm runs (the clock the device grants under this load); "not measured" without it.

Prints one JSON object; profiles/r07/match_see_net_rate.json holds a run.
    python profiles/experiments/match_see_net_rate.py [--n 8192] [--T 64] [--regions 5] [out.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402

from soccer2d_amd.actor import MatchQNetActor  # noqa: E402
from soccer2d_amd.match import MatchEngine  # noqa: E402

EPS = 0.1


class ClockSampler:
    """shader clock (MHz) of device 0 from `rocm-smi --showclocks`, sampled while a region runs"""

    def __init__(self):
        self.samples, self._stop, self._thread = [], threading.Event(), None

    def _run(self):
        while not self._stop.is_set():
            try:
                txt = subprocess.run(['rocm-smi', '-d', '0', '--showclocks'], capture_output=True, text=True, timeout=10).stdout
                m = re.search(r'sclk clock level: \d+: \((\d+)Mhz\)', txt)
                if m:
                    self.samples.append(int(m.group(1)))
            except Exception:
                return
            self._stop.wait(0.05)

    def __enter__(self):
        self._stop.clear()
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join()


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
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--launches', type=int, default=12)
    ap.add_argument('--loops', type=int, default=12)
    ap.add_argument('--warmup', type=float, default=1.0)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    n, T = a.n, a.T
    if not torch.cuda.is_available():
        raise SystemExit('match_see_net_rate.py measures on the GPU: no device found')
    torch.manual_seed(0)
    q = torch.nn.Sequential(torch.nn.Linear(192, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                            torch.nn.Linear(64, 16)).cuda()
    g = torch.Generator().manual_seed(1)
    table = torch.stack([torch.randint(1, 5, (16,), generator=g).float(), torch.rand(16, generator=g) * 200 - 100,
                         torch.rand(16, generator=g) * 360 - 180, torch.rand(16, generator=g) * 120 - 60,
                         torch.randint(0, 4, (16,), generator=g).float()], dim=1)
    actor = MatchQNetActor.from_module(q, table, epsilon=EPS, obs='see')
    res = {'device': torch.cuda.get_device_name(0), 'n': n, 'T': T, 'net': '192-64-64-16', 'slots': 22, 'epsilon': EPS, 'noise': True,
           'protocol': {'regions': a.regions, 'fused_launches_per_region': a.launches, 'unfused_loops_per_region': a.loops,
                        'warmup_seconds': a.warmup, 'arms': 'alternating'}}

    fused = MatchEngine(n, 'cuda:0', noise=True)
    fused.enable_vision()
    fused.set_network(actor)
    fused.reset()
    res['kernel'] = fused.kernel_name()
    out = fused.alloc_rollout(T, with_obs=False)
    out_rec = fused.alloc_rollout(T, with_obs=False)

    loose = MatchEngine(n, 'cuda:0', noise=True)
    loose.enable_vision()
    loose.reset()
    ro = loose.alloc_rollout(1, with_obs=False)
    rows = torch.empty((n, 22, 192), device='cuda:0')
    tab = table.cuda()

    def unfused():
        with torch.no_grad():
            for _ in range(T):
                x = loose.see('all', out=rows)
                idx = q(x).argmax(dim=2)
                explore = torch.rand(idx.shape, device='cuda:0') < EPS
                idx = torch.where(explore, torch.randint(0, 16, idx.shape, device='cuda:0'), idx)
                act = tab[idx]
                loose.rollout(1, actions=act[..., :3].unsqueeze(0), out=ro, with_obs=False)
                loose.vision_step(act[..., 3:], done=True)

    rows_eng = MatchEngine(n, 'cuda:0', noise=True)        # no network: a record-only launch builds and records the rows
    rows_eng.enable_vision()
    rows_eng.reset()
    out_rows = rows_eng.alloc_rollout(T, with_obs=False)

    arms = [('rows_only', lambda: rows_eng.rollout(T, out=out_rows, with_obs=False, see_obs='all'), a.launches),
            ('fused', lambda: fused.rollout(T, out=out, with_obs=False), a.launches),
            ('fused_see_record', lambda: fused.rollout(T, out=out_rec, with_obs=False, see_obs='all', net_index=True), a.launches),
            ('unfused_torch_loop', unfused, a.loops)]
    times = {name: [] for name, _, _ in arms}
    clock = ClockSampler()
    for name, fn, _ in arms:
        warm(fn, a.warmup)
    for _ in range(a.regions):
        for name, fn, count in arms:
            warm(fn, 0.1)                                  # back on this arm's code and clock after the other arms
            if name == 'fused':
                with clock:
                    times[name].append(region(fn, count))
            else:
                times[name].append(region(fn, count))
    for name, _, _ in arms:
        v = sorted(times[name])
        med = v[len(v) // 2]
        res[name] = {'seconds_per_T_cycles': {'median': med, 'min': v[0], 'max': v[-1], 'regions': times[name]},
                     'match_steps_per_s': {'median': n * T / med, 'min': n * T / v[-1], 'max': n * T / v[0]},
                     'agent_decisions_per_s': {'median': 22 * n * T / med, 'min': 22 * n * T / v[-1], 'max': 22 * n * T / v[0]}}
    del res['rows_only']['agent_decisions_per_s']           # (nobody decides there: the random policy)
    med = {name: res[name]['seconds_per_T_cycles']['median'] for name, _, _ in arms}
    res['speedup_fused_vs_unfused'] = med['unfused_torch_loop'] / med['fused']
    res['speedup_fused_see_record_vs_unfused'] = med['unfused_torch_loop'] / med['fused_see_record']
    res['see_record_cost'] = med['fused_see_record'] / med['fused']
    s = sorted(clock.samples)
    res['shader_clock_mhz_during_fused'] = ({'median': s[len(s) // 2], 'min': s[0], 'max': s[-1], 'samples': len(s)} if s
                                            else 'not measured')
    fused.close(); loose.close(); rows_eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
