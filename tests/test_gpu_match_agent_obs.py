"""Per-agent observations on the GPU (s2d_match_agent_obs): bit-exact to the host restatement (tests/agent_obs_ref.c) on the
engine's own states at full size, masks select exactly the matching rows, mirrored states give bitwise the same rows to the
mirrored agents, the call writes nothing else, and Soccer2DMatchVecEnv(obs='agent') returns them for self-play."""
import numpy as np
import pytest

import agent_obs as A
from soccer2d_amd import _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
N = 8192
TYPES = {t: {'player_speed_max': 1.05 + 0.01 * t, 'kickable_margin': 0.7 + 0.01 * t, 'player_size': 0.3 + 0.005 * t,
             'kick_power_rate': 0.027 + 0.0002 * t} for t in range(1, 17)}


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return A.build(tmp_path_factory.mktemp('agent_obs'))


def _engine(n, **kw):
    from soccer2d_amd.match import MatchEngine
    return MatchEngine(n, 'cuda:0', **kw)


def _state(eng):
    return {k: getattr(eng, k).cpu().numpy() for k in A.OBJ_PLANES + A.ENV_WORDS}


def _write(eng, s):
    for k in A.OBJ_PLANES + A.ENV_WORDS:
        getattr(eng, k).copy_(torch.from_numpy(np.ascontiguousarray(s[k])))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _assert_same(got, want, tag):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        e, p, k = bad[0]
        raise AssertionError(f'{tag}: {len(bad)} words differ; first match {e} agent row {p} word {k}: gpu={got[e, p, k]} '
                             f'host={want[e, p, k]}')


def _check(eng, ref, prm, tag):
    got = eng.agent_observations('all')
    torch.cuda.synchronize()
    _assert_same(got.cpu().numpy(), A.observations(ref, _state(eng), prm), tag)


CASES = {
    'random_noise': dict(kw=dict(noise=True), ctl=None),
    'scripted': dict(kw=dict(noise=True, seed=5), ctl={'left': 'scripted', 'right': 'scripted'}),
    'hetero': dict(kw=dict(noise=True, hetero_seed=3, player_type_id=[0] + [1, 2, 3, 4, 5, 6, 7, 8, 9, 10] + [0] + [11, 12, 13, 14, 15, 16, 17, 1, 2, 3]),
                   ctl=None),
    'general': dict(kw=dict(noise=True, half_time_cycles=40, nr_extra_halfs=1, extra_half_cycles=20, kickable_margin=0.8,
                            server_params={'ball_decay': 0.9, 'player_speed_max': 1.2}), ctl={'left': 'scripted', 'right': 'random'}),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_bit_exact_to_the_restatement(ref, case):
    c = CASES[case]
    eng = _engine(N, **c['kw'])
    if case == 'general':
        assert 'general' in eng.kernel_name() or 'own schedule' in eng.kernel_name()
    if c['ctl'] is not None:
        eng.set_controllers(c['ctl'])
    prm = A.params(eng.cfg)
    eng.reset()
    done = 0
    for t in (0, 1, 17, 64):
        if t > done:
            eng.rollout(t - done, with_obs=False)
            done = t
        _check(eng, ref, prm, f'{case} after {t} cycles')
    o = eng.agent_observations('all').cpu().numpy()
    assert (o[..., M.AGENT_OBS_FIELDS['game.self_reach_steps']] < M.REACH_NONE).any()
    eng.close()


def test_scenes_written_into_the_state(ref):
    """shoot-out modes, IllegalDefense_, red cards and a goalie holding the ball, written into the engine's planes"""
    eng = _engine(N, noise=True)
    prm = A.params(eng.cfg)
    eng.reset()
    eng.rollout(30, with_obs=False)
    rng = np.random.default_rng(1)
    s = _state(eng)
    modes = np.array([22, 23, 24, 25, 26, 27, 28, 29, 2, 3, 5, 6, 7, 21, 30, 10, 9, 8])
    s['mode'][:] = modes[np.arange(N) % len(modes)]
    s['mode_side'][:] = rng.integers(0, 3, N)
    s['card'][:, :22] = np.where(rng.random((N, 22)) < 0.08, M.CARD_RED, s['card'][:, :22])
    s['ball_holder'][:] = rng.choice([0, 1, 12], N)
    s['score_left'][:] = rng.integers(0, 5, N)
    s['cycle'][:] = rng.integers(0, 8000, N)
    _write(eng, s)
    o = eng.agent_observations('all').cpu().numpy()
    _assert_same(o, A.observations(ref, _state(eng), prm), 'scenes')
    pen = o[..., M.AGENT_OBS_FIELDS['game.is_penalty_kick_mode']]
    assert (pen[s['mode'] == 27] == 0).all() and (pen[s['mode'] == 28] == 1).all()
    eng.close()


@pytest.mark.parametrize('n', [1, 7, 8193])
def test_masks_select_rows(n):
    eng = _engine(n, noise=True)
    eng.reset()
    eng.rollout(9, with_obs=False)
    full = eng.agent_observations('all').cpu().numpy()
    assert full.shape == (n, 22, 224)
    for slots in ('left', 'right', 0x7FF, 0x3FF800, 0x2A5A5, 1 << 21, 1):
        mask = M.agent_slot_mask(slots)
        rows = [i for i in range(22) if (mask >> i) & 1]
        got = eng.agent_observations(slots).cpu().numpy()
        assert got.shape == (n, len(rows), 224)
        assert np.array_equal(_bits(got), _bits(full[:, rows])), slots
    out = torch.full((n, 11, 224), 7.0, device='cuda:0')
    assert eng.agent_observations('left', out=out) is out
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(full[:, :11]))
    for bad in (0, 1 << 22, 0x400000 | 1, 'middle'):
        with pytest.raises(ValueError):
            eng.agent_observations(bad)
    rc = eng.lib.s2d_match_agent_obs(eng._h, 1 << 22, out.data_ptr(), eng._stream())
    assert rc != 0                                        # the C side refuses the mask too ...
    assert eng.lib.s2d_match_agent_obs(eng._h, 0, out.data_ptr(), eng._stream()) != 0
    assert eng.lib.s2d_match_agent_obs(eng._h, 0x7FF, out.data_ptr() + 4, eng._stream()) != 0   # ... and an unaligned buffer
    eng.close()


def test_mirrored_states_give_mirrored_agents_the_same_rows(ref):
    ids = [0] + list(range(1, 11)) + [0] + list(range(7, 17))
    a = _engine(N, player_types=TYPES, player_type_id=ids)
    b = _engine(N, player_types=TYPES, player_type_id=ids[11:] + ids[:11])
    s = A.random_state(np.random.default_rng(9), N)
    _write(a, s)
    _write(b, A.mirror(s))
    oa = a.agent_observations('all').cpu().numpy()
    ob = b.agent_observations('all').cpu().numpy()
    assert np.array_equal(_bits(oa[:, :11]), _bits(ob[:, 11:]))
    assert np.array_equal(_bits(oa[:, 11:]), _bits(ob[:, :11]))
    _assert_same(oa, A.observations(ref, s, A.params(a.cfg)), 'random state')
    assert (oa[..., M.AGENT_OBS_FIELDS['self.is_kickable']] == 1).sum() > N // 8
    a.close(); b.close()


def test_reads_only():
    eng = _engine(N, noise=True)
    eng.reset()
    eng.rollout(5, with_obs=False)
    torch.cuda.synchronize()
    before = eng.arena.clone()
    eng.agent_observations('all')
    eng.agent_observations(0x2A5A5)
    torch.cuda.synchronize()
    assert torch.equal(before, eng.arena)
    eng.close()


def test_vec_env_self_play():
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    n = 512
    env = Soccer2DMatchVecEnv(n, obs='agent', noise=True)
    assert env.observation_space.shape == (22, 224) and env.action_space.shape == (22, 3)
    obs = env.reset()
    assert obs.shape == (n, 22, 224)
    assert torch.equal(obs, env.engine.agent_observations('all'))
    g = torch.Generator(device='cuda:0').manual_seed(4)
    goals = 0
    for _ in range(70):
        a = torch.empty((n, 22, 3), device='cuda:0')
        a[..., 0] = torch.randint(0, 5, (n, 22), device='cuda:0', generator=g).float()
        a[..., 1] = torch.rand((n, 22), device='cuda:0', generator=g) * 200 - 100
        a[..., 2] = torch.rand((n, 22), device='cuda:0', generator=g) * 360 - 180
        obs, rew, done, info = env.step(a)
        assert obs.shape == (n, 22, 224) and rew.shape == (n, 22)
        assert torch.equal(obs, env.engine.agent_observations('all'))
        rl = env.engine.reward_left
        assert torch.equal(rew[:, :11], rl[:, None].expand(n, 11)) and torch.equal(rew[:, 11:], -rl[:, None].expand(n, 11))
        goals += int((rl != 0).sum())
    env.close()
    env = Soccer2DMatchVecEnv(64, opponent='scripted', obs='agent')
    assert env.reset().shape == (64, 11, 224)
    obs, rew, done, info = env.step(torch.zeros((64, 11, 3), device='cuda:0'))
    assert obs.shape == (64, 11, 224) and rew.shape == (64, 11)
    assert torch.equal(obs, env.engine.agent_observations('left'))
    env.close()
    env = Soccer2DMatchVecEnv(64)
    assert env.reset().shape == (64, 23, 5) and env.step(None)[0].shape == (64, 23, 5)
    env.close()
