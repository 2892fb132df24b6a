"""Cost of the per-agent observations (s2d_match_agent_obs) at 8 192 matches: kernel time and achieved write bandwidth for the
full mask (22 agents) and the left team (0x7FF), against the algorithmic bytes N * k * 896; and Soccer2DMatchVecEnv.step per
second with obs='state' and obs='agent' (self-play, caller actions).  Median of 5 regions after a 2 s settle.
--quick: a few launches of each mask only (for the rocprofv3 kernel-trace and counter runs)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gym-soccer-2d-env_amd')]
import torch  # noqa: E402
from soccer2d_amd.match import MatchEngine, Soccer2DMatchVecEnv  # noqa: E402

N, L, R = 8192, 200, 5


def regions(fn, per_region):
    end = time.time() + 2.0
    while time.time() < end:
        fn()
        torch.cuda.synchronize()
    out = []
    for _ in range(R):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_region):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / per_region)
    return sorted(out)[R // 2], out


def main():
    quick = '--quick' in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    eng = MatchEngine(N, 'cuda:0', noise=True)
    eng.reset()
    eng.rollout(40, with_obs=False)
    lines = [f'# {torch.cuda.get_device_name(0)}; {N} matches; kernel: median of {R} regions of {L} launches; '
             f'env: {R} regions of 100 steps']
    for label, slots, k in (('full mask (22 agents)', 'all', 22), ('left team (0x7FF)', 'left', 11)):
        out = torch.empty((N, k, 224), dtype=torch.float32, device='cuda:0')
        if quick:
            for _ in range(20):
                eng.agent_observations(slots, out=out)
            torch.cuda.synchronize()
            continue
        med, all_ = regions(lambda: eng.agent_observations(slots, out=out), L)
        nbytes = N * k * 896
        lines.append(f'agent_obs {label:22s} {med * 1e6:8.2f} us  {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e12:5.2f} TB/s  '
                     'regions ' + ' '.join(f'{t * 1e6:.2f}' for t in all_))
        print(lines[-1], flush=True)
    eng.close()
    if quick:
        return
    for obs in ('state', 'agent'):
        env = Soccer2DMatchVecEnv(N, obs=obs, noise=True)
        env.reset()
        a = torch.zeros((N, 22, 3), dtype=torch.float32, device='cuda:0')
        a[..., 0] = 1.0
        a[..., 1] = 50.0
        med, all_ = regions(lambda: env.step(a), 100)
        lines.append(f"Soccer2DMatchVecEnv(obs='{obs}').step {1.0 / med:10.0f} steps/s  {med * 1e6:8.2f} us/step  "
                     'regions ' + ' '.join(f'{t * 1e6:.2f}' for t in all_))
        print(lines[-1], flush=True)
        env.close()
    if args:
        open(args[0], 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
