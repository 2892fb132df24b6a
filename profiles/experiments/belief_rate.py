"""The belief layer (MatchEngine.belief_step / belief_scan: s2d_match_belief_scan) at 8 192 matches x 22 agents, beside the
s2d_match_see call that writes the rows it reads, in ONE process, on see rows of a played match (scripted against scripted, noise
on, random TurnNeck / ChangeView every cycle).

  see             MatchEngine.see('all'): the 180 224 see rows of the current state.
  belief_step     one update (T = 1) with one of the 64 recorded rows per agent, the rows taken in turn.
  belief_scan     T = 64 updates in one launch over the whole record, state only.
  belief_scan_out the same with the belief after every row recorded.

Protocol: every arm is warmed up for `--warmup` seconds of back-to-back work (past the clock ramp that follows an idle gap), then
`--regions` timed regions per arm, the arms alternating; a region is a number of calls (sized to about `--region-seconds`)
between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and the highest, in
microseconds per call; the bytes the call must move -- per agent 768 B of see row in, 768 B of state in and 768 B of state out
per launch, plus 768 B per recorded row (see: 768 B out) -- over the median time, as a fraction of an 8 TB/s roofline; and the
shader clock the device reports while the scan runs (read only; null where it cannot be read).  No threshold: the numbers are
reported.

Prints one JSON object; profiles/r22/belief_rate.json holds a run.
    python profiles/experiments/belief_rate.py [--regions 5] [out.json]"""
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

from soccer2d_amd.match import MatchEngine  # noqa: E402

ROW_BYTES = 768
ROOFLINE = 8.0e12


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
    return mhz[0] if mhz else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--matches', type=int, default=8192)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--region-seconds', type=float, default=0.3)
    ap.add_argument('--warmup', type=float, default=0.5)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('belief_rate.py measures on the GPU: no device found')
    dev, N, T = 'cuda:0', a.matches, a.steps
    agents = N * 22
    eng = MatchEngine(N, dev, noise=True, seed=22)
    eng.set_controllers({'left': 'scripted', 'right': 'scripted'})
    eng.enable_vision()
    eng.enable_belief('all')
    eng.reset()
    g = torch.Generator(device=dev).manual_seed(22)
    record = torch.empty((T, N, 22, 192), dtype=torch.float32, device=dev)
    for t in range(T):                                     # the played record
        v = torch.empty((N, 22, 2), device=dev)
        v[..., 0] = torch.rand((N, 22), device=dev, generator=g) * 180 - 90
        v[..., 1] = torch.randint(0, 4, (N, 22), device=dev, generator=g).float() * (torch.rand((N, 22), device=dev, generator=g) < 0.3)
        eng.step(None)
        eng.vision_step(v, done=True)
        eng.see('all', out=record[t])
    out = torch.empty_like(record)
    rows = torch.empty((N, 22, 192), dtype=torch.float32, device=dev)
    turn = [0]

    def step():
        eng.belief_step(record[turn[0] % T])
        turn[0] += 1

    arms = [('see', lambda: eng.see('all', out=rows), ROW_BYTES),
            ('belief_step', step, 3 * ROW_BYTES),
            ('belief_scan', lambda: eng.belief_scan(record), (T + 2) * ROW_BYTES),
            ('belief_scan_out', lambda: eng.belief_scan(record, out=out), (2 * T + 2) * ROW_BYTES)]
    res = {'device': torch.cuda.get_device_name(0), 'matches': N, 'agents': agents, 'T': T, 'row_bytes': ROW_BYTES,
           'roofline_bytes_per_s': ROOFLINE,
           'protocol': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    fresh = record[..., 8].mean().item()
    res['record'] = {'fresh_share': fresh, 'seen_player_rows_per_fresh_row': (record[..., 24::8] >= 1).sum().item() / max(1.0, fresh * T * agents),
                     'level_1_to_3_share_of_seen': ((record[..., 24::8] >= 1) & (record[..., 24::8] <= 3)).sum().item()
                     / max(1, (record[..., 24::8] >= 1).sum().item())}
    times, counts = {k: [] for k, _, _ in arms}, {}
    for k, fn, _ in arms:
        warm(fn, a.warmup)
        counts[k] = max(3, int(a.region_seconds / region(fn, 3)))
    res['sclk_mhz_while_busy'] = busy_clock_mhz(arms[2][1], 20 * counts['belief_scan'])
    for _ in range(a.regions):
        for k, fn, _ in arms:
            warm(fn, 0.05)                                 # back on this arm's code and clock after the other arms
            times[k].append(region(fn, counts[k]))
    for k, _, per_agent in arms:
        v = sorted(times[k])
        med = v[len(v) // 2]
        res[k] = {'us_per_call': {'median': med * 1e6, 'min': v[0] * 1e6, 'max': v[-1] * 1e6, 'regions': [x * 1e6 for x in times[k]]},
                  'calls_per_region': counts[k], 'bytes_per_call_counted': per_agent * agents,
                  'bytes_per_s_of_the_counted_traffic': per_agent * agents / med,
                  'fraction_of_roofline': per_agent * agents / med / ROOFLINE}
    res['belief_step_over_see'] = res['belief_step']['us_per_call']['median'] / res['see']['us_per_call']['median']
    res['belief_scan_us_per_row'] = res['belief_scan']['us_per_call']['median'] / T
    known = (eng.belief[..., 29::8] < eng.belief_params.count_max).float().mean().item()
    res['known_player_entries_at_the_end'] = known
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
