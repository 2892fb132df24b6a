"""Episode statistics on the device (soccer2d_amd.episodes.EpisodeStats.update: s2d_episode_stats) against the two ways the tree
had to learn which episodes ended in a [T, N] record, in ONE process, on synthetic records of 65 536 x 256 and 4 096 x 64 with
about 0.5 % and 5 % of the steps ending an episode.

  update          EpisodeStats.update(reward, done, result): five launches, no host read.  Eager and as a graph replay.
  callback        InfoCollectorCallback.on_result_codes(result): a device-wide nonzero, a synchronising copy and one Python
                  dict per episode.  It yields the results only (no return, no length).
  torch           the same outputs in torch: a bincount of the results where done, and episode returns and lengths from a
                  segmented cumsum over T (cumsum, the row of the previous done by cummax, a gather), the carries advanced, the
                  mean over the last 100 episodes read on the host -- its synchronisation is part of the time, as it is part of
                  SB3's logging.  Different summation order, so returns agree to rounding, not bitwise; the counts are equal.

Protocol: every arm is warmed up for `--warmup` seconds of back-to-back work (past the clock ramp that follows an idle gap), then
`--regions` timed regions per arm, the arms alternating; a region is a number of calls (sized to about `--region-seconds`)
between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and the highest, in
seconds per call; the ratios of the medians; the bytes the three passes must move (done once in the count pass; reward, done and
result in the scatter pass: 7 B per step) over the update's time; and the shader clock the device reports while the update runs
(read only; null where it cannot be read).

Prints one JSON object; profiles/r20/episode_stats_rate.json holds a run.
    python profiles/experiments/episode_stats_rate.py [--regions 5] [out.json]"""
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

from soccer2d_amd.episodes import EpisodeStats  # noqa: E402
from utils.info_collector_callback import InfoCollectorCallback  # noqa: E402

SHAPES = ((65536, 256), (4096, 64))
RATES = (0.005, 0.05)
BYTES_PER_STEP = 7


class TorchStats:
    """the torch formulation: carries, counts and the last `window` returns and lengths"""

    def __init__(self, N, window, device):
        self.acc_return = torch.zeros(N, device=device)
        self.acc_length = torch.zeros(N, dtype=torch.int64, device=device)
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)
        self.window = window
        self.returns = torch.zeros(0, device=device)
        self.lengths = torch.zeros(0, dtype=torch.int64, device=device)

    def update(self, reward, done, result):
        T, N = done.shape
        d = done.bool()
        self.counts += torch.bincount(result[d].long(), minlength=4)[:4]
        cs = reward.cumsum(0) + self.acc_return[None]
        t = torch.arange(1, T + 1, device=done.device)[:, None].expand(T, N)          # steps taken up to and including row t
        last = torch.where(d, t, torch.zeros_like(t)).cummax(0).values                  # ... up to the latest done, 0 if none
        prev = torch.cat([torch.zeros_like(last[:1]), last[:-1]])                       # the same, before this row
        base = torch.where(prev > 0, cs.gather(0, (prev - 1).clamp(min=0)), torch.zeros_like(cs))
        ret = (cs - base)[d]                                                           # row-major: the order of the ring
        length = (t - prev + torch.where(prev == 0, self.acc_length[None].expand(T, N), torch.zeros_like(prev)))[d]
        tail = last[-1]
        self.acc_return = torch.where(tail > 0, cs[-1] - cs.gather(0, (tail - 1).clamp(min=0)[None])[0], cs[-1])
        self.acc_length = torch.where(tail > 0, T - tail, self.acc_length + T)
        self.returns = torch.cat([self.returns, ret])[-self.window:]
        self.lengths = torch.cat([self.lengths, length])[-self.window:]
        return float(self.returns.mean()) if self.returns.numel() else float('nan')    # the host read SB3's logger makes


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
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
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
    return mhz[0] if mhz else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--region-seconds', type=float, default=0.3)
    ap.add_argument('--warmup', type=float, default=0.5)
    ap.add_argument('--capacity', type=int, default=100)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('episode_stats_rate.py measures on the GPU: no device found')
    dev = 'cuda:0'
    res = {'device': torch.cuda.get_device_name(0), 'capacity': a.capacity, 'bytes_per_step_counted': BYTES_PER_STEP,
           'protocol': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup, 'arms': 'alternating'},
           'configurations': []}
    for (N, T), rate in ((s, r) for s in SHAPES for r in RATES):
        g = torch.Generator(device=dev).manual_seed(N + T)
        done = (torch.rand((T, N), device=dev, generator=g) < rate).to(torch.uint8)
        reward = torch.randn((T, N), device=dev, generator=g)
        result = (done * torch.randint(1, 4, (T, N), device=dev, generator=g)).to(torch.uint8)
        n = int(done.sum())
        st, gst, ts, cb = EpisodeStats(N, a.capacity, dev), EpisodeStats(N, a.capacity, dev), TorchStats(N, a.capacity, dev), \
            InfoCollectorCallback()
        gst.workspace(T, N)

        def callback():
            cb.reset()
            cb.on_result_codes(result)

        arms = [('update', lambda: st.update(reward, done, result)), ('update_graph', captured(lambda: gst.update(reward, done, result))),
                ('callback_on_result_codes', callback), ('torch_formulation', lambda: ts.update(reward, done, result))]
        entry = {'num_envs': N, 'T': T, 'done_rate': rate, 'episodes_per_record': n, 'record_bytes_counted': BYTES_PER_STEP * T * N}
        times, counts = {k: [] for k, _ in arms}, {}
        for k, fn in arms:
            warm(fn, a.warmup)
            counts[k] = max(3, int(a.region_seconds / region(fn, 3)))
        entry['sclk_mhz_while_busy'] = busy_clock_mhz(arms[1][1], 20 * counts['update_graph'])
        for _ in range(a.regions):
            for k, fn in arms:
                warm(fn, 0.05)                                 # back on this arm's code and clock after the other arms
                times[k].append(region(fn, counts[k]))
        med = {}
        for k, _ in arms:
            v = sorted(times[k])
            med[k] = v[len(v) // 2]
            entry[k] = {'seconds_per_call': {'median': med[k], 'min': v[0], 'max': v[-1], 'regions': times[k]}, 'calls_per_region': counts[k]}
        for k in ('update', 'update_graph'):
            entry[k]['steps_per_s'] = T * N / med[k]
            entry[k]['bytes_per_s_of_the_counted_traffic'] = BYTES_PER_STEP * T * N / med[k]
        entry['callback_over_update'] = med['callback_on_result_codes'] / med['update']
        entry['torch_over_update'] = med['torch_formulation'] / med['update']
        entry['torch_over_update_graph'] = med['torch_formulation'] / med['update_graph']

        # the same episodes: one update from a zero state against the torch formulation from a zero state
        a1, t1 = EpisodeStats(N, max(1, n), dev).update(reward, done, result), TorchStats(N, max(1, n), dev)
        t1.update(reward, done, result)
        ep, tot = a1.episodes(), a1.totals.cpu().tolist()
        entry['counts_equal_torch'] = tot[2:6] == t1.counts.cpu().tolist() and tot[0] == n
        entry['lengths_equal_torch'] = bool(torch.equal(ep['length'].long(), t1.lengths))
        entry['largest_return_difference_from_torch'] = float((ep['return'] - t1.returns).abs().max()) if n else 0.0
        res['configurations'].append(entry)
        del done, reward, result, st, gst, ts
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
