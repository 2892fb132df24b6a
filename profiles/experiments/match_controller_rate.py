"""Rate of the 11v11 engine with in-kernel controllers: 8 192 matches, stock rules, T = 64 cycles per launch with the usual
rollout record (obs, reward, mode, done), match-steps/s.  Rows: no table (the random policy: today's kernel), both teams
scripted, scripted vs random, and both scripted with the action record.  Median of 5 regions of 16 launches after a 2 s settle."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gym-soccer-2d-env_amd')]
import torch  # noqa: E402
from soccer2d_amd.match import MatchEngine  # noqa: E402

N, T, L, R = 8192, 64, 16, 5


def measure(ctl, record):
    eng = MatchEngine(N, 'cuda:0')
    if ctl is not None:
        eng.set_controllers(ctl)
    eng.reset()
    out = eng.alloc_rollout(T, True, record)
    end = time.time() + 2.0
    while time.time() < end:
        eng.rollout(T, out=out, record_actions=record)
        torch.cuda.synchronize()
    rates = []
    for _ in range(R):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(L):
            eng.rollout(T, out=out, record_actions=record)
        b.record()
        torch.cuda.synchronize()
        rates.append(N * T * L / (a.elapsed_time(b) * 1e-3))
    name = eng.kernel_name()
    eng.close()
    return sorted(rates)[R // 2], rates, name


if __name__ == '__main__':
    rows = [('no table (random)', None, False), ('scripted vs scripted', [2] * 22, False),
            ('scripted vs random', {'left': 'scripted', 'right': 'random'}, False), ('scripted vs scripted + record', [2] * 22, True)]
    lines = [f'# {torch.cuda.get_device_name(0)}; {N} matches x {T} cycles per launch, {L} launches per region, {R} regions, median']
    for label, ctl, rec in rows:
        med, rates, name = measure(ctl, rec)
        lines.append(f'{label:32s} {med / 1e6:8.2f} M match-steps/s  regions ' + ' '.join(f'{r / 1e6:.2f}' for r in rates) + f'  {name}')
        print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], 'w').write('\n'.join(lines) + '\n')
