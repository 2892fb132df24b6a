"""11v11 league play: learner versus a frozen opponent, each on its own 224-64-64-16 network, at 8192 matches, T = 64 cycles per
launch, stock rules, noise on.  Four arms, two libraries, one session:

  (a) parent_one_network   the parent commit's library, one network on all 22 slots (the README's network-slots line)
  (b) one_network          this commit's library, the same launch (must stay within the spread of (a))
  (c) two_networks         this commit: network A on the left team, opponent network B on the right, one launch per T cycles
  (d) parent_unfused       the parent: A in the kernel on the left team, B evaluated by torch on agent_observations('right')
                           every cycle (agent rows -> torch MLP -> argmax -> epsilon -> gather from the table -> rollout(1))

The parent's library is built from the parent commit (`git worktree add`, `make -C gym-soccer-2d-env_amd/csrc`) and given with
--parent-lib; without it (a) and (d) are "not measured".  One process can hold only one libs2d_hip.so, so each library runs in a
worker process of this script; the driver alternates the arms between the two workers.

Protocol: every arm is warmed up for `--warmup` seconds of back-to-back work (past the clock ramp that follows an idle gap), then
`--regions` timed regions per arm, the arms alternating; a region is `--launches` fused launches (or `--loops` unfused loops of T
cycles) between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and the
highest, as seconds per T cycles, match-steps/s and agent decisions/s; the ratios (b)/(a), (c)/(b) and (d)/(c) of the medians.
The shader clock is sampled with `rocm-smi --showclocks` while (b) runs (the clock the device grants under this load).

Prints one JSON object; profiles/r08/match_two_nets_rate.json holds a run.
    python profiles/experiments/match_two_nets_rate.py --parent-lib PATH [--n 8192] [--T 64] [--regions 5] [out.json]"""
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

EPS_A, EPS_B = 0.05, 0.0


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


# ---------------------------------------------------------------- worker: one library, its arms, commands on stdin
def worker(role, n, T):
    import torch
    from soccer2d_amd import _capi, _capi_match as M
    lib = _capi.load_library()                             # S2D_LIB: the library of this worker
    # the parent's library has no opponent network: bind what it exports
    M.MATCH_PROTOTYPES = tuple(p for p in M.MATCH_PROTOTYPES if hasattr(lib, p[0]))
    from soccer2d_amd.actor import MatchQNetActor
    from soccer2d_amd.match import MatchEngine

    def module(seed):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(224, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                                   torch.nn.Linear(64, 16)).cuda()

    def table(seed):
        g = torch.Generator().manual_seed(seed)
        return torch.stack([torch.randint(1, 5, (16,), generator=g).float(), torch.rand(16, generator=g) * 200 - 100,
                            torch.rand(16, generator=g) * 360 - 180], dim=1)

    qa, qb = module(0), module(1)
    ta, tb = table(1), table(2)
    a = MatchQNetActor.from_module(qa, ta, epsilon=EPS_A)
    b = MatchQNetActor.from_module(qb, tb, epsilon=EPS_B)
    arms, names = {}, {}

    one = MatchEngine(n, 'cuda:0', noise=True)
    one.set_network(a)
    one.reset()
    out_one = one.alloc_rollout(T, with_obs=False)
    if role == 'parent':
        arms['parent_one_network'] = lambda: one.rollout(T, out=out_one, with_obs=False)
        names['parent_one_network'] = one.kernel_name()
        loose = MatchEngine(n, 'cuda:0', noise=True)
        loose.set_controllers({'left': 'external', 'right': 'external'})
        loose.set_network(a, 'left')
        loose.reset()
        ro = loose.alloc_rollout(1, with_obs=False)
        rows = torch.empty((n, 11, 224), device='cuda:0')
        act = torch.zeros((1, n, 22, 3), device='cuda:0')
        tab = tb.cuda()

        def unfused():
            with torch.no_grad():
                for _ in range(T):
                    x = loose.agent_observations('right', out=rows)
                    idx = qb(x).argmax(dim=2)
                    explore = torch.rand(idx.shape, device='cuda:0') < EPS_B
                    idx = torch.where(explore, torch.randint(0, 16, idx.shape, device='cuda:0'), idx)
                    act[0, :, 11:] = tab[idx]
                    loose.rollout(1, actions=act, out=ro, with_obs=False)
        arms['parent_unfused'] = unfused
        names['parent_unfused'] = loose.kernel_name()
    else:
        arms['one_network'] = lambda: one.rollout(T, out=out_one, with_obs=False)
        names['one_network'] = one.kernel_name()
        two = MatchEngine(n, 'cuda:0', noise=True)
        two.set_network(a, 'left')
        two.set_opponent_network(b, 'right')
        two.reset()
        out_two = two.alloc_rollout(T, with_obs=False)
        arms['two_networks'] = lambda: two.rollout(T, out=out_two, with_obs=False)
        names['two_networks'] = two.kernel_name()
    torch.cuda.synchronize()
    print(json.dumps({'ready': names, 'device': torch.cuda.get_device_name(0)}), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == 'quit':
            break
        fn = arms[cmd[1]]
        if cmd[0] == 'warm':
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < float(cmd[2]):
                fn()
                torch.cuda.synchronize()
            print(json.dumps({'ok': True}), flush=True)
        else:                                              # region NAME COUNT
            count = int(cmd[2])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(count):
                fn()
            torch.cuda.synchronize()
            print(json.dumps({'seconds': (time.perf_counter() - t0) / count}), flush=True)


# ---------------------------------------------------------------- driver
class Worker:
    def __init__(self, role, lib, n, T):
        env = dict(os.environ)
        if lib:
            env['S2D_LIB'] = os.path.abspath(lib)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', role, '--n', str(n), '--T', str(T)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        self.ready = None

    def read(self):
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit(f'a worker ended early (exit status {self.p.wait()})')
        return json.loads(line)

    def ask(self, *words):
        self.p.stdin.write(' '.join(str(w) for w in words) + '\n')
        self.p.stdin.flush()
        return self.read()

    def close(self):
        try:
            self.p.stdin.write('quit\n')
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--launches', type=int, default=24)
    ap.add_argument('--loops', type=int, default=12)
    ap.add_argument('--warmup', type=float, default=1.0)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    n, T = a.n, a.T
    if a.worker:
        return worker(a.worker, n, T)
    workers = {'this': Worker('this', None, n, T)}
    if a.parent_lib:
        if not os.path.exists(a.parent_lib):
            raise SystemExit(f'{a.parent_lib} not found')
        workers['parent'] = Worker('parent', a.parent_lib, n, T)
    res = {'n': n, 'T': T, 'net': '224-64-64-16 (A: epsilon %g, B: epsilon %g)' % (EPS_A, EPS_B), 'noise': True,
           'protocol': {'regions': a.regions, 'fused_launches_per_region': a.launches, 'unfused_loops_per_region': a.loops,
                        'warmup_seconds': a.warmup, 'arms': 'alternating, one worker process per library'}, 'kernel': {}}
    arms = []
    try:
        for role, w in workers.items():
            w.ready = w.read()
            res['device'] = w.ready['device']
            res['kernel'].update(w.ready['ready'])
        order = ['parent_one_network', 'one_network', 'two_networks', 'parent_unfused']
        for name in order:
            for role, w in workers.items():
                if name in w.ready['ready']:
                    arms.append((name, w, a.loops if name == 'parent_unfused' else a.launches))
        times = {name: [] for name, _, _ in arms}
        clock = ClockSampler()
        for name, w, _ in arms:
            w.ask('warm', name, a.warmup)
        for _ in range(a.regions):
            for name, w, count in arms:
                w.ask('warm', name, 0.1)                   # back on this arm's code and clock after the other arms
                if name == 'one_network':
                    with clock:
                        times[name].append(w.ask('region', name, count)['seconds'])
                else:
                    times[name].append(w.ask('region', name, count)['seconds'])
    finally:
        for w in workers.values():
            w.close()
    med = {}
    for name, _, _ in arms:
        v = sorted(times[name])
        med[name] = v[len(v) // 2]
        res[name] = {'seconds_per_T_cycles': {'median': med[name], 'min': v[0], 'max': v[-1], 'regions': times[name]},
                     'match_steps_per_s': {'median': n * T / med[name], 'min': n * T / v[-1], 'max': n * T / v[0]},
                     'agent_decisions_per_s': {'median': 22 * n * T / med[name], 'min': 22 * n * T / v[-1], 'max': 22 * n * T / v[0]}}
    for name in ('parent_one_network', 'parent_unfused'):
        res.setdefault(name, 'not measured')
    res['two_networks_vs_one_network_time'] = med['two_networks'] / med['one_network']
    if 'parent' in workers:
        res['one_network_vs_parent_time'] = med['one_network'] / med['parent_one_network']
        res['one_network_within_parent_spread'] = bool(med['one_network'] <= res['parent_one_network']['seconds_per_T_cycles']['max'])
        res['speedup_two_networks_vs_parent_unfused'] = med['parent_unfused'] / med['two_networks']
    s = sorted(clock.samples)
    res['shader_clock_mhz_during_one_network'] = ({'median': s[len(s) // 2], 'min': s[0], 'max': s[-1], 'samples': len(s)} if s
                                                  else 'not measured')
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
