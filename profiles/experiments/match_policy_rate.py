"""11v11 self-play with a stochastic policy in the cycle kernel (policy slots, s2d_match_set_policy_network) at 8192 matches,
T = 64 cycles per launch, 224-64-64-16 on all 22 slots, stock rules, noise on.  Five arms, two libraries, one session:

  (a) policy_relu / policy_tanh   this commit: the policy launch with log-probabilities recorded, either hidden activation
  (b) qnet                        this commit's library, the Q-network launch (must stay within the spread of (c))
  (c) parent_qnet                 the parent commit's library, the same launch
  (d) unfused_categorical         this commit: agent_observations('all') -> torch MLP (Tanh) -> torch.distributions.Categorical
                                  sample and log_prob -> gather from the table -> rollout(1), once per cycle

The parent's library is built from the parent commit (`git worktree add`, `make -C gym-soccer-2d-env_amd/csrc`) and given with
--parent-lib; without it (c) is "not measured".  One process can hold only one libs2d_hip.so, so each library runs in a worker
process of this script; the driver alternates the arms between the two workers.

Protocol: every arm is warmed up for `--warmup` seconds of back-to-back work (past the clock ramp that follows an idle gap), then
`--regions` timed regions per arm, the arms alternating; a region is `--launches` fused launches (or `--loops` unfused loops of T
cycles) between two host clocks that end in a device synchronise.  Reported per arm: the median region, the lowest and the
highest, as seconds per T cycles, match-steps/s and agent decisions/s; the ratios policy/(b), policy/(d) and (b)/(c) of the
medians, and whether (b)'s median lies within max - min of (c)'s regions around (c)'s median.  The shader clock is sampled with
`rocm-smi --showclocks` while the tanh policy arm runs (the clock the device grants under this load).

Prints one JSON object; profiles/r08/match_policy_rate.json holds a run.
    python profiles/experiments/match_policy_rate.py --parent-lib PATH [--n 8192] [--T 64] [--regions 5] [out.json]"""
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

EPS = 0.05


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
    # the parent's library has no policy slots: bind what it exports
    M.MATCH_PROTOTYPES = tuple(p for p in M.MATCH_PROTOTYPES if hasattr(lib, p[0]))
    from soccer2d_amd.actor import MatchQNetActor
    from soccer2d_amd.match import MatchEngine

    def module(seed, act):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(224, 64), act(), torch.nn.Linear(64, 64), act(), torch.nn.Linear(64, 16)).cuda()

    g = torch.Generator().manual_seed(1)
    table = torch.stack([torch.randint(1, 5, (16,), generator=g).float(), torch.rand(16, generator=g) * 200 - 100,
                         torch.rand(16, generator=g) * 360 - 180], dim=1)
    arms, names = {}, {}

    def fused(name, actor, **kw):
        eng = MatchEngine(n, 'cuda:0', noise=True)
        eng.set_network(actor)
        eng.reset()
        out = eng.alloc_rollout(T, with_obs=False)
        arms[name] = lambda: eng.rollout(T, out=out, with_obs=False, **kw)
        arms[name]()                                       # (allocates the records)
        names[name] = eng.kernel_name()

    q = MatchQNetActor.from_module(module(0, torch.nn.ReLU), table, epsilon=EPS)
    if role == 'parent':
        fused('parent_qnet', q)
    else:
        from soccer2d_amd.actor import MatchPolicyActor
        fused('qnet', q)
        fused('policy_relu', MatchPolicyActor.from_module(module(0, torch.nn.ReLU), table), logp=True, net_index=True)
        pi = module(0, torch.nn.Tanh)
        fused('policy_tanh', MatchPolicyActor.from_module(pi, table), logp=True, net_index=True)
        loose = MatchEngine(n, 'cuda:0', noise=True)
        loose.set_controllers({'left': 'external', 'right': 'external'})
        loose.reset()
        ro = loose.alloc_rollout(1, with_obs=False)
        rows = torch.empty((n, 22, 224), device='cuda:0')
        act = torch.zeros((1, n, 22, 3), device='cuda:0')
        logp = torch.empty((T, n, 22), device='cuda:0')
        index = torch.empty((T, n, 22), dtype=torch.int64, device='cuda:0')
        tab = table.cuda()

        def unfused():
            with torch.no_grad():
                for t in range(T):
                    d = torch.distributions.Categorical(logits=pi(loose.agent_observations('all', out=rows)))
                    idx = d.sample()
                    index[t], logp[t] = idx, d.log_prob(idx)
                    act[0] = tab[idx]
                    loose.rollout(1, actions=act, out=ro, with_obs=False)
        arms['unfused_categorical'] = unfused
        names['unfused_categorical'] = loose.kernel_name()
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
    res = {'n': n, 'T': T, 'net': '224-64-64-16 on all 22 slots (Q-network: epsilon %g)' % EPS, 'noise': True,
           'protocol': {'regions': a.regions, 'fused_launches_per_region': a.launches, 'unfused_loops_per_region': a.loops,
                        'warmup_seconds': a.warmup, 'arms': 'alternating, one worker process per library'}, 'kernel': {}}
    arms = []
    try:
        for role, w in workers.items():
            w.ready = w.read()
            res['device'] = w.ready['device']
            res['kernel'].update(w.ready['ready'])
        order = ['parent_qnet', 'qnet', 'policy_relu', 'policy_tanh', 'unfused_categorical']
        for name in order:
            for role, w in workers.items():
                if name in w.ready['ready']:
                    arms.append((name, w, a.loops if name == 'unfused_categorical' else a.launches))
        times = {name: [] for name, _, _ in arms}
        clock = ClockSampler()
        for name, w, _ in arms:
            w.ask('warm', name, a.warmup)
        for _ in range(a.regions):
            for name, w, count in arms:
                w.ask('warm', name, 0.1)                   # back on this arm's code and clock after the other arms
                if name == 'policy_tanh':
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
    res.setdefault('parent_qnet', 'not measured')
    for arm in ('policy_relu', 'policy_tanh'):
        res[arm + '_vs_qnet_time'] = med[arm] / med['qnet']
        res['speedup_' + arm + '_vs_unfused_categorical'] = med['unfused_categorical'] / med[arm]
    if 'parent' in workers:
        p = res['parent_qnet']['seconds_per_T_cycles']
        res['qnet_vs_parent_time'] = med['qnet'] / med['parent_qnet']
        res['parent_spread_seconds'] = p['max'] - p['min']
        res['qnet_within_parent_spread'] = bool(abs(med['qnet'] - med['parent_qnet']) <= p['max'] - p['min'])
    s = sorted(clock.samples)
    res['shader_clock_mhz_during_policy_tanh'] = ({'median': s[len(s) // 2], 'min': s[0], 'max': s[-1], 'samples': len(s)} if s
                                                  else 'not measured')
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
