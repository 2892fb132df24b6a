"""The observation KERNELS (s2d_match_relative, s2d_match_agent_obs, s2d_match_see) against the plain float64 reference of
tests/obs_f64.py, by its rule: states written into the engine's planes (random, heterogeneous types, a second vision parameter
set, slot masks) and states reached by play; the constructed edge scenes both against float64 and bit for bit against the fp32
restatements, with their known answers; egocentric_tables against float64 and against the agent rows' bearing words."""
import numpy as np
import pytest

import agent_obs as A
import match_see as S
import obs_f64 as F
from soccer2d_amd import _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

OTHER = dict(view_angle=(45.0, 90.0, 200.0), see_interval=(1.0, 3.0, 4.0), visible_distance=5.0, dist_quantize_step=0.05,
             dist_round=0.01, dist_chg_quantize=0.05, dir_chg_quantize=0.5, unum_far_length=10.0, unum_too_far_length=25.0,
             team_far_length=30.0, team_too_far_length=70.0)
SCHED = dict(half_time_cycles=6, nr_extra_halfs=1, extra_half_cycles=4, kick_off_wait=2, after_goal_wait=3, drop_ball_time=20,
             announce_wait=4, pen_before_setup_wait=2, pen_ready_wait=3, pen_taken_wait=12, pen_nr_kicks=2, pen_max_extra_kicks=2)
HETERO = dict(hetero_seed=3, player_type_id=[0] + [1, 2, 3, 4, 5, 6, 7, 8, 9, 10] + [0] + [11, 12, 13, 14, 15, 16, 17, 1, 2, 3])
ENGINE_KEYS = A.OBJ_PLANES + A.ENV_WORDS + ('tick',)


@pytest.fixture(scope='module')
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp('obs_f64')
    return A.build(d), S.build(d)


def _engine(n, vision=None, **kw):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(n, 'cuda:0', **kw)
    eng.enable_vision(**(vision or {}))
    return eng


def _write(eng, s):
    for k in F.STATE_KEYS:
        getattr(eng, k).copy_(torch.from_numpy(np.ascontiguousarray(s[k])))


def _state(eng):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).cpu().numpy() for k in F.STATE_KEYS}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _kernels(eng, mask='all'):
    agent, see = eng.agent_observations(mask).cpu().numpy(), eng.see(mask).cpu().numpy()
    dist, angle = (t.cpu().numpy() for t in eng.relative_tables())
    return agent, see, dist, angle


def _check(eng, vp, cap, tag, mask='all'):
    """the three kernels on the engine's current state against float64; returns (state, agent rows, see rows, dist, angle)"""
    state = _state(eng)
    n = eng.num_envs
    agent, see, dist, angle = _kernels(eng, mask)
    bits = M.agent_slot_mask(mask)
    ids = eng.cfg.env_id_offset + np.arange(n)
    for kind, (rep, fails) in (('agent', F.compare_agent(state, eng.cfg, agent, bits)),
                               ('see', F.compare_see(state, vp, eng.cfg.seed, ids, see, bits)),
                               ('relative', F.compare_relative(state, dist, angle))):
        print(f'{tag}: {kind}: ill {rep["ill"]} of {rep["n"]} rows ({100 * rep["share"]:.3f} %), worst excess (ulps) '
              + ', '.join(f'{k} {v:.2f}' for k, v in rep['worst'].items()))
        assert not fails, f'{tag}: {kind}: ' + '\n'.join(fails[:10])
        assert rep['share'] <= cap, (tag, kind, rep['ill'], rep['n'])
    return state, agent, see, dist, angle


class Coverage:
    """what the compared rows contained (full-mask rows)"""

    def __init__(self, vp):
        self.V, self.seen = F.vision_values(vp), set()

    def add(self, agent, see):
        V, rows = self.V, see[..., 24:].reshape(see.shape[:2] + (21, 8))
        lv, d = rows[..., 0], rows[..., 3]
        self.seen |= {f'level {int(k)}' for k in np.unique(lv)} | {f'ball level {int(k)}' for k in np.unique(see[..., 16])}
        for name, lo, hi, kept in (('unum', V['unum_far_length'], V['unum_too_far_length'], 4),
                                   ('team', V['team_far_length'], V['team_too_far_length'], 3)):
            inside = (lv >= 2) & (d > lo + 0.1 * (hi - lo)) & (d < hi - 0.1 * (hi - lo))       # the seen distance is a grid point near d
            self.seen |= {f'{name} band kept'} if (inside & (lv >= kept)).any() else set()
            self.seen |= {f'{name} band lost'} if (inside & (lv < kept)).any() else set()
        q = np.concatenate([rows[..., 3:8].reshape(see.shape[:2] + (-1,)), see[..., 17:21]], axis=-1)
        if (np.signbit(q) & (q == 0)).any():
            self.seen.add('-0 quantised word')
        if (lv == 1).any() or (see[..., 16] == 1).any():
            self.seen.add('felt outside the cone')
        r = agent[..., M.AGENT_OBS_FIELDS['game.self_reach_steps']]
        self.seen |= {name for name, hit in (('reach 0', r == 0), ('reach between', (r > 0) & (r < M.REACH_NONE)),
                                             ('reach NONE', r == M.REACH_NONE)) if hit.any()}
        if (agent[..., M.AGENT_OBS_FIELDS['self.is_kickable']] == 1).any():
            self.seen.add('kickable agent')

    WANT = ({f'level {k}' for k in range(5)} | {'unum band kept', 'unum band lost', 'team band kept', 'team band lost',
                                                 '-0 quantised word', 'felt outside the cone', 'reach 0', 'reach between',
                                                 'reach NONE', 'kickable agent'})

    def check(self, tag):
        print(f'{tag}: saw {sorted(self.seen)}')
        assert self.WANT <= self.seen, (tag, sorted(self.WANT - self.seen))


@pytest.mark.parametrize('n', [1, 9, 1024])
def test_random_states(n):
    """one match per half-wave, 8 per block: one match, a ragged last block, and 1 024 for the statistics"""
    eng = _engine(n, seed=40 + n, env_id_offset=3 * n)
    _write(eng, F.random_state(np.random.default_rng(200 + n), n))
    _, agent, see, _, _ = _check(eng, {}, F.ILL_CAP, f'random n={n}')
    if n >= 1024:
        cov = Coverage({})
        cov.add(agent, see)
        cov.check('random')
    eng.close()


@pytest.mark.parametrize('case,kw,vp', [('hetero', HETERO, {}), ('other vision', {}, OTHER)])
def test_other_types_and_parameters(case, kw, vp):
    n = 256
    eng = _engine(n, vision=vp, **kw)
    _write(eng, F.random_state(np.random.default_rng(7), n, vp))
    _, agent, see, _, _ = _check(eng, vp, F.ILL_CAP, case)
    cov = Coverage(vp)
    cov.add(agent, see)
    cov.check(case)
    eng.close()


def test_states_reached_by_play():
    """64 cycles of the scripted team against the random policy with noise, view actions drawn per cycle, under a short schedule
    with the clocks started next to the ends of the periods: half time, extra time and the shoot-out fall inside the run.  The
    shoot-out parks the waiting players on a 1.5 m grid, every second neighbour exactly on the default visible_distance of 3 m,
    and a neck on its clamp of +-90 faces exactly along that grid: half the rows of a batch would sit on a threshold.  So these
    states are seen with visible_distance = 3.25, and each TurnNeck goes to a random angle inside the clamp."""
    n = 256
    vp = dict(visible_distance=3.25)
    eng = _engine(n, vision=vp, noise=True, seed=13, **SCHED)
    eng.set_controllers({'left': 'scripted', 'right': 'random'})
    eng.reset()
    g = torch.Generator(device='cpu').manual_seed(11)
    ends = torch.tensor((0, 6, 12, 16), dtype=torch.int32)[torch.randint(0, 4, (n,), generator=g)]
    eng.cycle.copy_((ends - torch.randint(1, 4, (n,), generator=g, dtype=torch.int32)).clamp(min=0).to(eng.device))
    cov, modes = Coverage(vp), set()
    for t in range(1, 65):
        eng.rollout(1, with_obs=False)
        v = torch.zeros((n, 22, 2))
        v[..., 0] = torch.rand((n, 22), generator=g) * 170 - 85 - eng.neck[:, :22].cpu()
        v[..., 1] = torch.randint(0, 4, (n, 22), generator=g).float() * (torch.rand((n, 22), generator=g) < 0.3)
        eng.vision_step(v.to(eng.device), done=True)
        if t in (2, 9, 30, 64):
            state, agent, see, _, _ = _check(eng, vp, F.ILL_CAP, f'play, cycle {t}')
            cov.add(agent, see)
            modes |= set(np.unique(state['mode']).tolist())
    cov.check('play')
    assert {M.GM_PLAY_ON, M.GM_KICK_OFF} <= modes and modes & set(M.PENALTY_MODES), sorted(modes)
    assert (state['cycle'] > 12).any()                    # extra time was played
    eng.close()


@pytest.mark.parametrize('mask', [0x2A5A5, 'left', 'right', 1 << 21])
def test_slot_masks(mask):
    n = 64
    eng = _engine(n, seed=77)
    _write(eng, F.random_state(np.random.default_rng(8), n))
    _, agent, see, _, _ = _check(eng, {}, F.ILL_CAP, f'mask {mask}', mask)
    k = bin(M.agent_slot_mask(mask)).count('1')
    assert agent.shape == (n, k, 224) and see.shape == (n, k, 192)
    eng.close()


@pytest.mark.parametrize('case,kw,vp', [('default', {}, None), ('other vision, hetero', HETERO, OTHER)])
def test_edge_scenes(libs, case, kw, vp):
    """the constructed scenes on the device: against float64 under the edge cap, bit for bit against the fp32 restatements (the
    bitwise GPU tests never run these inputs), and their known answers"""
    probe = _engine(1, vision=vp, **kw)                   # (the scenes are built for the engine's own configuration)
    state, known = F.edge_scenes(probe.cfg, vp)
    probe.close()
    n = len(state['mode'])
    eng = _engine(n, vision=vp, **kw)
    _write(eng, state)
    back = _state(eng)
    assert all(np.array_equal(back[k], state[k]) for k in F.STATE_KEYS)
    _, agent, see, dist, angle = _check(eng, vp or {}, F.EDGE_ILL_CAP, f'edges, {case}')
    bad = F.check_known(known, agent, see, dist, angle)
    assert not bad, '\n'.join(bad[:10])
    want_agent = A.observations(libs[0], state, A.params(eng.cfg))
    want_see = S.see(libs[1], state, S.params(seed=eng.cfg.seed, env_id_offset=eng.cfg.env_id_offset, **(vp or {})))
    for kind, got, want in (('agent', agent, want_agent), ('see', see, want_see)):
        diff = np.argwhere(_bits(got) != _bits(want))
        assert not len(diff), (f'{kind} rows: {len(diff)} words differ from the restatement; first (match, agent, word) '
                               f'{tuple(diff[0])}: gpu={got[tuple(diff[0])]!r} host={want[tuple(diff[0])]!r}')
    eng.close()


def test_egocentric_tables():
    """the bearing of egocentric_tables against float64 by the rule (objects that wrap at +-180 included), and against the agent
    rows' bearing words of the same state within the same tolerance"""
    n = 256
    eng = _engine(n)
    rng = np.random.default_rng(9)
    s = F.random_state(rng, n)
    for e, (body, ang) in enumerate(((179.0, -179.0), (-179.0, 179.0), (180.0, -90.0), (-180.0, 90.0), (90.0, -90.0), (0.0, 180.0))):
        s['x'][e, 0], s['y'][e, 0], s['body'][e, 0] = 0.0, 0.0, body   # agent 0 at the origin: the ball at direction `ang`
        s['x'][e, 22], s['y'][e, 22] = np.float32(10.0 * np.cos(np.radians(ang))), np.float32(10.0 * np.sin(np.radians(ang)))
    _write(eng, s)
    t = eng.egocentric_tables()
    ego = t['bearing'].cpu().numpy()
    agent = eng.agent_observations('all').cpu().numpy()
    rep, fails = F.compare_bearings(s, ego)
    print(f'egocentric: worst excess {rep["worst"]}')
    assert not fails, '\n'.join(fails[:10])
    assert (ego > -180.0).all() and (ego <= 180.0).all()
    _, angle = F.relative(s)
    raw = angle - s['body'][:, :22, None].astype(np.float64)
    assert (np.abs(raw) > 180.0).mean() > 0.2                # the wrap is exercised
    assert abs(abs(ego[2, 0, 22]) - 90.0) < 1e-3 and abs(abs(ego[0, 0, 22]) - 2.0) < 1e-3 and abs(abs(ego[5, 0, 22]) - 180.0) < 1e-3
    rows = F.row_bearings(agent)
    active = s['card'][:, :22] < M.CARD_RED
    both = np.concatenate([active, np.ones((n, 1), bool)], axis=1)[:, None, :] & np.ones((1, 22, 1), bool)
    d = np.abs(ego.astype(np.float64) - rows)
    d = np.minimum(d, np.abs(360.0 - d))
    allowed = F.T_ULPS['bearing'] * F.UNIT['bearing'] + 2.0 * rep['spread']
    bad = np.argwhere(both & (d > allowed))
    assert not len(bad), (len(bad), tuple(bad[0]), ego[tuple(bad[0])], rows[tuple(bad[0])])
    dist, _ = eng.relative_tables()
    assert torch.equal(t['dist'], dist)
    eng.close()
