"""The 11v11 match KERNEL against the fp64 libm build of its oracle: every device buffer of a state is copied into the fp64 oracle,
the device runs one cycle through rollout_ex with the action record (so the in-kernel random and scripted controllers' choices are
known), the fp64 oracle steps with the recorded actions, and the two are compared by the rule of tests/match_f64.py.  Every
instantiation of the cycle kernel, with and without controllers; checkpoints in early play, set plays, extra time and the
shoot-out; the constructed edge states written into the device planes."""
import numpy as np
import pytest

import match_f64 as F
import match_oracle as MO
from soccer2d_amd import _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

N = 8192
# the largest ill-conditioned fraction accepted in one checkpoint (the CPU corpus of tests/test_match_oracle_f64.py measures 0 in
# play; a few matches of 8 192 may sit on a threshold)
ILL_CAP = 0.005
EDGE_ILL_CAP = 0.15
SCHED = dict(half_time_cycles=6, nr_extra_halfs=1, extra_half_cycles=4, kick_off_wait=2, after_goal_wait=3, drop_ball_time=20,
             announce_wait=4, pen_before_setup_wait=2, pen_ready_wait=3, pen_taken_wait=12, pen_nr_kicks=2, pen_max_extra_kicks=2)
TYPE_IDS = [0] + [1 + i for i in range(10)] + [0] + [17 - i for i in range(10)]
# the ends of the periods (half time, normal time, extra time) of the stock schedule and of SCHED: every match's clock starts a few
# cycles before one of them (or at 0), so that half time, extra time and the shoot-out fall inside the checkpoints
STOCK_ENDS, SCHED_ENDS = (0, 3000, 6000, 8000), (0, 6, 12, 16)
# (instantiation, configuration, period ends)
KERNELS = [('stock, stock types', {}, STOCK_ENDS),
           ('stock', dict(hetero_seed=5, player_type_id=TYPE_IDS), STOCK_ENDS),
           ('stock rules, own schedule', dict(SCHED), SCHED_ENDS),
           ('general', dict(SCHED, tackle_cycles=8), SCHED_ENDS),
           ('general, illegal defense', dict(SCHED, illegal_defense_number=1, illegal_defense_duration=3, illegal_defense_dist_x=30.0),
            SCHED_ENDS)]
CHECKPOINTS = (0, 1, 4, 9, 15, 22, 30, 45)          # device cycles after the reset at which one cycle is compared
SHOOT_OUT = {M.GM_PENALTY_ONFIELD, M.GM_PENALTY_SETUP, M.GM_PENALTY_READY}


def _engines(n, noise=False, **kw):
    from soccer2d_amd.match import MatchEngine, make_match_config
    hetero = dict(hetero_seed=kw.pop('hetero_seed', None), player_type_id=kw.pop('player_type_id', None))
    cfg = make_match_config(noise=noise, **hetero, **kw)
    eng = MatchEngine(n, 'cuda:0', cfg=cfg)
    ocfg = MO.make_match_config(noise=int(noise), player_type_id=hetero['player_type_id'], **kw)
    for t in range(M.MATCH_PLAYER_TYPES):                # the type table is input data: the oracle gets the device's
        ocfg.player_types[t] = cfg.player_types[t]
    return eng, ocfg


def _device_state(eng):
    torch.cuda.synchronize()
    return {name: getattr(eng, name).cpu().numpy().copy() for name in MO.STATE_FIELDS}


def _write_state(eng, state):
    for name in MO.STATE_FIELDS:
        getattr(eng, name).copy_(torch.as_tensor(state[name], device=eng.device))
    torch.cuda.synchronize()


def _one_cycle(eng, ocfg, actions=None, ill_cap=ILL_CAP, tag=''):
    """one device cycle from the device's state, compared with the fp64 oracle; returns (modes before and after, events of the cycle)"""
    before = _device_state(eng)
    a = None if actions is None else torch.as_tensor(actions, device=eng.device).reshape(1, eng.num_envs, 22, 3)
    out = eng.rollout(1, actions=a, with_obs=False, record_actions=True)
    rec = out['actions'][0].cpu().numpy()
    after = _device_state(eng)
    ids = ocfg.env_id_offset + np.arange(eng.num_envs)
    rep, fails = F.compare(ocfg, before, rec, ids, after)
    assert not fails, f'{tag}: ' + '\n'.join(fails[:10])
    assert rep['ill'] <= ill_cap * eng.num_envs, (tag, rep['ill'], rep['ill_words'])
    _, ev = F.f32_step(ocfg, before, rec, ids)           # (the device equals the fp32 oracle bit for bit: its events are the device's)
    return set(np.unique(before['mode']).tolist()) | set(np.unique(after['mode']).tolist()), ev


@pytest.mark.parametrize('controllers', [None, {'left': 'scripted', 'right': 'random'}], ids=['no-table', 'controllers'])
@pytest.mark.parametrize('name,kw,ends', KERNELS, ids=[k[0] for k in KERNELS])
def test_kernel_one_cycle_matches_f64(name, kw, ends, controllers):
    eng, ocfg = _engines(N, noise=controllers is not None, **kw)
    if controllers is not None:
        eng.set_controllers(controllers)
    want = f'<{name}, controllers>' if controllers is not None else f'<{name}>'
    assert eng.kernel_name() == 's2d_match_rollout_kernel' + want
    g = torch.Generator(device='cpu').manual_seed(11)     # clocks next to half time, the end of normal time, of extra time
    end = torch.tensor(ends, dtype=torch.int32)[torch.randint(0, len(ends), (N,), generator=g)]
    lead = torch.randint(1, 12 if ends[1] > 100 else 4, (N,), generator=g, dtype=torch.int32)
    eng.cycle.copy_((end - lead).clamp(min=0).to(eng.device))
    modes, events = set(), 0
    done = 0
    for c in CHECKPOINTS:
        if c > done:
            eng.rollout(c - done, with_obs=False)
        m, ev = _one_cycle(eng, ocfg, tag=f'{name} {controllers} cycle {c}')
        modes |= m
        events |= int(np.bitwise_or.reduce(ev))
        done = c + 1
    assert {M.GM_PLAY_ON, M.GM_KICK_OFF, M.GM_FIRST_HALF_OVER, M.GM_EXTEND_HALF} <= modes, sorted(modes)
    assert SHOOT_OUT <= modes, sorted(modes)
    assert events & MO.EV_KICK and events & MO.EV_COLLIDE, events


@pytest.mark.parametrize('noise', [False, True])
def test_edge_states_on_device_match_f64(noise):
    """the constructed edge states of tests/match_f64.py written into the device planes, one cycle, compared with fp64"""
    state, a = F.edge_states()
    n = len(a)
    eng, ocfg = _engines(n, noise=noise)
    assert eng.kernel_name() == 's2d_match_rollout_kernel<stock, stock types>'
    _write_state(eng, state)
    assert all(np.array_equal(v, state[k]) for k, v in _device_state(eng).items())
    modes, ev = _one_cycle(eng, ocfg, actions=a, ill_cap=EDGE_ILL_CAP, tag=f'edges noise={noise}')
    assert (ev & MO.EV_CATCH).any() and (ev & MO.EV_KICK).any() and (ev & MO.EV_TACKLE).any()
