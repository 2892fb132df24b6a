"""Cost of the movement-noise models on the bench's workload, in ONE process: noise off, the lattice (noise_model='lattice', the
default) and rcssserver's uniform square (noise_model='rcssserver').  Each configuration runs bench.py's rollout measurement --
65 536 envs x 256 fused cycles per launch, the discrete random policy, rotating record buffers (> 600 MiB in flight), graph replay,
a settle phase past the clock ramp, then five timed regions of `--steps` launches, the median reported -- through bench.py's own
functions, so that the three figures are what `bench.py [--noise]` would print for them.  The lattice and the square run a second
time in the opposite order, so that a drift of the box shows up as a difference between the two passes.

  python profiles/experiments/noise_model_cost.py [--envs 65536] [--fuse 256] [--steps 32]
"""
import argparse
import gc
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402  (puts the package and tests/ on sys.path)


def measure(model, n, T, steps, settle_ms):
    import torch
    from soccer2d_amd.engine import Engine, make_config
    noise = model != 'off'
    cfg = make_config(seed=0x5EED, noise=noise, noise_model='lattice' if model == 'off' else model, **B.DQN_KWARGS)
    eng = Engine(n, 'cuda:0', cfg=cfg)
    eng.reset()
    stream = torch.cuda.current_stream()
    nbuf = B.n_rotating(T * n * B.RECORD_BYTES)
    m = B.measure_rollout(eng, T, steps, nbuf, B.REPEATS, stream, settle_ms)
    e = B.rollout_entry(m, n, T, eng.kernel_name(), None)
    r = e['roofline']
    row = {'model': model, 'env_steps_per_s': e['value'], 'launch_us': r['launch_us'], 'launch_us_events': r.get('launch_us_events'),
           'hbm_frac': r['frac'], 'kernel': eng.kernel_name(), 'repeats': e['repeats'], 'buffers': nbuf}
    del eng, m
    gc.collect()
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--fuse', type=int, default=256)
    ap.add_argument('--steps', type=int, default=32, help='launches per timed region (bench.py --steps)')
    ap.add_argument('--settle-ms', type=float, default=200.0)
    a = ap.parse_args()
    import torch
    print(f"# {torch.cuda.get_device_name(0)}; {a.envs} envs x {a.fuse} fused cycles per launch, {a.steps} launches per region, "
          f"{B.REPEATS} regions, median; discrete random policy (bench.py's workload)")
    rows = [measure(m, a.envs, a.fuse, a.steps, a.settle_ms) for m in ('off', 'lattice', 'rcssserver', 'rcssserver', 'lattice')]
    for r in rows:
        print(f"{r['model']:>10}  {r['env_steps_per_s'] / 1e9:7.2f} G env-steps/s  {r['launch_us']:8.1f} us/launch "
              f"(events {r['launch_us_events']:8.1f})  HBM {100 * r['hbm_frac']:5.1f} %  "
              f"regions {' '.join(f'{v / 1e9:.2f}' for v in r['repeats'])}  {r['kernel']}")
    by = {}
    for r in rows:
        by.setdefault(r['model'], []).append(r['env_steps_per_s'])
    lat, sq = max(by['lattice']), max(by['rcssserver'])
    print(f"rcssserver / lattice = {sq / lat:.3f} (best of two passes each; per pass: "
          f"{by['rcssserver'][0] / by['lattice'][0]:.3f}, {by['rcssserver'][1] / by['lattice'][1]:.3f}); "
          f"lattice / off = {lat / by['off'][0]:.3f}")


if __name__ == '__main__':
    main()
