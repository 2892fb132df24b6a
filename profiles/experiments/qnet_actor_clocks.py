"""Where a wave-cycle of the fused Q-network actor spends its clocks: the network (observation tile, three MFMA layers, argmax)
against the rest of the cycle (action draw, simulation, record stores), from the s_memtime stamps of an experiment build.

    make -C gym-soccer-2d-env_amd/csrc OUT=$PWD/gym-soccer-2d-env_amd/lib/stamps EXTRA=-DS2D_QNET_STAMPS
    S2D_LIB=$PWD/gym-soccer-2d-env_amd/lib/stamps/libs2d_hip.so python profiles/experiments/qnet_actor_clocks.py

Each wave's lane 0 writes its sums (network, rest, prologue, whole kernel) into terminal_obs row wave_first of the arena; the
figures below are medians and maxima over the waves of one launch, divided by T for the per-cycle numbers."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'gym-soccer-2d-env_amd')):
    sys.path.insert(0, p)

import torch  # noqa: E402

from soccer2d_amd.actor import QNetActor  # noqa: E402
from soccer2d_amd.engine import Engine, make_config  # noqa: E402

DQN = dict(change_ball_position=True, change_ball_velocity=True, min_distance_to_ball=5.0, max_steps=200,
           use_continuous_action=False, action_space_size=16, use_turning=False)
MFMA_PER_WAVE_CYCLE = 4 * (4 * 3 + 4 * 16 + 1 * 16)   # 10-64-64-16: four 16-env tiles x (layer 1 + layer 2 + layer 3)


def run(n, T, noise):
    assert 'stamps' in os.environ.get('S2D_LIB', ''), 'needs the -DS2D_QNET_STAMPS build in S2D_LIB'
    eng = Engine(n, 'cuda:0', cfg=make_config(noise=noise, **DQN))
    eng.reset()
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                              torch.nn.Linear(64, 16)).cuda()
    actor = QNetActor.from_module(net, epsilon=0.05)
    out = eng.alloc_rollout(T, terminal_obs=True)
    eng.rollout_qnet(T, actor, out=out)          # warm
    eng.rollout_qnet(T, actor, out=out)
    torch.cuda.synchronize()
    st = eng.terminal_obs[::64, :4].double().cpu()
    med, mx = st.median(dim=0).values.tolist(), st.max(dim=0).values.tolist()
    return {'envs': n, 'T': T, 'noise': noise, 'waves': st.shape[0], 'kernel': eng.kernel_name(),
            'clocks_per_wave_cycle_median': {'network': med[0] / T, 'rest_of_cycle': med[1] / T},
            'clocks_per_wave_cycle_max': {'network': mx[0] / T, 'rest_of_cycle': mx[1] / T},
            'prologue_clocks_median': med[2], 'kernel_clocks_median': med[3], 'kernel_clocks_max': mx[3],
            'mfma_issue_floor_per_wave_cycle': MFMA_PER_WAVE_CYCLE * 32,
            'network_share_median': med[0] / max(1.0, med[3])}


def main():
    res = {'device': torch.cuda.get_device_name(0),
           'fused_65536_T256_noise_off': run(65536, 256, False),
           'fused_65536_T256_lattice': run(65536, 256, True),
           'fused_4096_T256_noise_off': run(4096, 256, False)}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
