"""The vision layer on the GPU (s2d_match_see, s2d_match_vision_step, s2d_match_vision_reset): bit-exact to the host restatement
(tests/see_ref.c) on random states and on a played match, the three vision planes word for word over that match, nothing written
but the output, rows a pure function of state and tick, Soccer2DMatchVecEnv(obs='see'), and an engine without vision unchanged
against the CPU match oracle."""
import numpy as np
import pytest

import match_oracle as MO
import match_see as S
from soccer2d_amd import _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
MASKS = ('all', 'left', 'right', 1, 1 << 10, 1 << 11, 1 << 21, 0x2A5A5)


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return S.build(tmp_path_factory.mktemp('see_ref'))


def _engine(n, vision=None, **kw):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(n, 'cuda:0', **kw)
    if vision is not None:
        eng.enable_vision(**vision)
    return eng


def _prm(eng, **vision):
    return S.params(seed=eng.cfg.seed, env_id_offset=eng.cfg.env_id_offset, **vision)


def _state(eng):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).cpu().numpy() for k in S.ENGINE_KEYS + S.VISION_PLANES}


def _write(eng, s):
    for k in S.ENGINE_KEYS + S.VISION_PLANES:
        getattr(eng, k).copy_(torch.from_numpy(np.ascontiguousarray(s[k])))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _assert_same(got, want, tag):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        e, p, k = bad[0]
        raise AssertionError(f'{tag}: {len(bad)} words differ; first match {e} agent row {p} word {k}: gpu={got[e, p, k]!r} '
                             f'host={want[e, p, k]!r}')


@pytest.mark.parametrize('n,kw', [(1, {}), (7, dict(seed=99, env_id_offset=5)), (8193, dict(seed=3))])
def test_bit_exact_on_random_states(ref, n, kw):
    eng = _engine(n, vision={}, **kw)
    prm = _prm(eng)
    s = S.random_state(np.random.default_rng(100 + n), n, prm)
    _write(eng, s)
    full = eng.see('all').cpu().numpy()
    assert full.shape == (n, 22, 192)
    want = S.see(ref, s, prm)
    _assert_same(full, want, f'n={n} all')
    for slots in MASKS:
        mask = M.agent_slot_mask(slots)
        rows = [i for i in range(22) if (mask >> i) & 1]
        got = eng.see(slots).cpu().numpy()
        assert got.shape == (n, len(rows), 192)
        _assert_same(got, want[:, rows], f'n={n} mask {slots}')
    if n > 1000:                                          # every level, both bands, every width occur
        lv = full[:, :, 24::8]
        assert all((lv == k).sum() > 100 for k in range(5)) and all((full[:, :, 7] == w).any() for w in (1, 2, 3))
        assert (full[:, :, 16] == 4).any() and (full[:, :, 16] == 1).any() and (full[:, :, 8] == 0).any()
    out = torch.full((n, 11, 192), 7.0, device='cuda:0')
    assert eng.see('left', out=out) is out
    _assert_same(out.cpu().numpy(), want[:, :11], 'out=')
    eng.close()


def test_other_parameters(ref):
    over = dict(view_angle=(45.0, 90.0, 200.0), see_interval=(1.0, 3.0, 4.0), visible_distance=5.0, dist_quantize_step=0.05,
                dist_round=0.01, dist_chg_quantize=0.05, dir_chg_quantize=0.5, unum_far_length=10.0, unum_too_far_length=25.0,
                team_far_length=30.0, team_too_far_length=70.0)
    n = 2048
    eng = _engine(n, vision=over)
    prm = _prm(eng, **over)
    s = S.random_state(np.random.default_rng(5), n, prm)
    _write(eng, s)
    _assert_same(eng.see('all').cpu().numpy(), S.see(ref, s, prm), 'other parameters')
    eng.close()


def test_played_match(ref):
    """64 played cycles, noise on, random body and view actions, short halves (matches end and restart): the vision planes equal
    the restatement's after every cycle, the see rows on the engine's own states at ticks > 0"""
    n, T = 512, 64
    eng = _engine(n, vision={}, noise=True, seed=11, half_time_cycles=15, nr_extra_halfs=0, penalty_shoot_outs=0)
    prm = _prm(eng)
    eng.reset()
    rng = np.random.default_rng(6)
    planes = {k: v for k, v in _state(eng).items() if k in S.VISION_PLANES}
    assert (planes['view_width'] == 2).all() and not planes['neck'].any() and not planes['see_wait'].any()
    finished = 0
    for t in range(T):
        a = np.zeros((n, 22, 3), dtype=np.float32)
        a[..., 0] = rng.integers(0, 5, (n, 22))
        a[..., 1] = rng.uniform(-100, 100, (n, 22))
        a[..., 2] = rng.uniform(-180, 180, (n, 22))
        v = np.zeros((n, 22, 2), dtype=np.float32)
        v[..., 0] = rng.uniform(-200, 200, (n, 22))
        v[..., 0][rng.random((n, 22)) < 0.02] = np.nan
        v[..., 1] = rng.integers(0, 5, (n, 22)) * (rng.random((n, 22)) < 0.3)
        eng.step(torch.from_numpy(a).cuda())
        eng.vision_step(torch.from_numpy(v).cuda(), done=True)
        s = _state(eng)
        done = eng.done.cpu().numpy()
        finished += int(done.sum())
        planes = S.vision_step(ref, dict(s, **planes), prm, v, done)
        for k in S.VISION_PLANES:
            assert np.array_equal(_bits(s[k]), _bits(planes[k])), (t, k)
        if t % 8 == 7 or t < 3:
            assert (s['tick'] > 0).all()
            _assert_same(eng.see('all').cpu().numpy(), S.see(ref, s, prm), f'cycle {t}')
    assert finished > 0
    o = eng.see('all').cpu().numpy()
    assert (o[:, :, 8] == 1).any() and (o[:, :, 8] == 0).any() and (o[:, :, 5] != 0).any()
    eng.close()


def test_reads_only():
    n = 4096
    eng = _engine(n, vision={}, noise=True)
    eng.reset()
    eng.rollout(5, with_obs=False)
    eng.vision_step()
    torch.cuda.synchronize()
    arena = eng.arena.clone()
    planes = [getattr(eng, k).clone() for k in S.VISION_PLANES]
    eng.see('all')
    eng.see(0x2A5A5)
    torch.cuda.synchronize()
    assert torch.equal(arena, eng.arena)
    assert all(torch.equal(a, getattr(eng, k)) for a, k in zip(planes, S.VISION_PLANES))
    v = torch.zeros((n, 22, 2), device='cuda:0')
    v[..., 0], v[..., 1] = 30.0, 3.0
    eng.vision_step(v, done=True)
    torch.cuda.synchronize()
    assert torch.equal(arena, eng.arena)                  # the engine's buffers are not the vision step's to write
    assert (eng.neck[:, :22] == 30.0).all() and (eng.view_width[:, :22] == 3).all()
    assert (eng.neck[:, 22:] == 0).all() and (eng.view_width[:, 22:] == 2).all()
    eng.close()


def test_pure_function_of_state_and_tick():
    n = 4096
    eng = _engine(n, vision={}, noise=True)
    eng.reset()
    eng.rollout(40, with_obs=False)
    eng.vision_step()
    a = eng.see('all').cpu().numpy()
    b = eng.see('all').cpu().numpy()
    assert np.array_equal(_bits(a), _bits(b))
    eng.tick.add_(1)
    c = eng.see('all').cpu().numpy()
    diff = _bits(a) != _bits(c)
    assert diff.any()
    assert not diff[:, :, :24].any()                      # self, ball and game words do not depend on the tick
    rows_a, rows_c = a[:, :, 24:].reshape(n, 22, 21, 8), c[:, :, 24:].reshape(n, 22, 21, 8)
    assert np.array_equal(_bits(rows_a[..., 3:5]), _bits(rows_c[..., 3:5]))      # dist and dir: the rows stay where they are
    changed = diff[:, :, 24:].reshape(n, 22, 21, 8).any(axis=3)
    dist = rows_a[..., 3][changed]
    assert (dist > 19.5).all() and (dist < 61.0).all()    # only identities inside a band (20..40, 40..60) can change
    assert (rows_a[..., 0][changed] != rows_c[..., 0][changed]).all()
    eng.close()


def test_errors():
    eng = _engine(4)
    with pytest.raises(RuntimeError):
        eng.see('all')
    with pytest.raises(RuntimeError):
        eng.vision_step()
    eng.enable_vision()
    for bad in (0, 1 << 22, 'middle'):
        with pytest.raises(ValueError):
            eng.see(bad)
    with pytest.raises(ValueError):
        eng.vision_step(torch.zeros((4, 22, 3), device='cuda:0'))
    with pytest.raises(ValueError):
        eng.enable_vision(see_interval=(0, 2, 3))
    import ctypes as C
    out = torch.zeros((4, 22, 192), device='cuda:0')
    args = (C.byref(eng.vision_params), C.byref(eng.vision))
    assert eng.lib.s2d_match_see(eng._h, *args, 1 << 22, out.data_ptr(), eng._stream()) != 0
    assert eng.lib.s2d_match_see(eng._h, *args, 0, out.data_ptr(), eng._stream()) != 0
    assert eng.lib.s2d_match_see(eng._h, *args, 0x7FF, out.data_ptr() + 4, eng._stream()) != 0
    assert eng.lib.s2d_match_see(eng._h, *args, 0x7FF, None, eng._stream()) != 0
    assert eng.lib.s2d_match_see(eng._h, *args, 0x3FFFFF, out.data_ptr(), eng._stream()) == 0
    eng.close()


def test_vec_env_see():
    from soccer2d_amd.match import MatchEngine, Soccer2DMatchVecEnv
    n = 256
    kw = dict(noise=True, seed=21, half_time_cycles=12, nr_extra_halfs=0, penalty_shoot_outs=0)
    env = Soccer2DMatchVecEnv(n, obs='see', **kw)
    assert env.observation_space.shape == (22, 192) and env.action_space.shape == (22, 5)
    hand = MatchEngine(n, 'cuda:0', **kw)
    hand.enable_vision()
    obs = env.reset()
    hand.reset()
    assert obs.shape == (n, 22, 192) and torch.equal(obs, hand.see('all'))
    assert not obs[:, :, 24:].any() and (obs[:, :, 8] == 0).all()            # a reset row is not fresh
    g = torch.Generator(device='cuda:0').manual_seed(4)
    restarted = 0
    for t in range(40):
        a = torch.empty((n, 22, 5), device='cuda:0')
        a[..., 0] = torch.randint(0, 5, (n, 22), device='cuda:0', generator=g).float()
        a[..., 1] = torch.rand((n, 22), device='cuda:0', generator=g) * 200 - 100
        a[..., 2] = torch.rand((n, 22), device='cuda:0', generator=g) * 360 - 180
        a[..., 3] = torch.rand((n, 22), device='cuda:0', generator=g) * 120 - 60
        a[..., 4] = torch.randint(0, 4, (n, 22), device='cuda:0', generator=g).float()
        obs, rew, done, info = env.step(a)
        assert obs.shape == (n, 22, 192) and rew.shape == (n, 22)
        hand.step(a[..., :3].contiguous())                # the three calls by hand
        hand.vision_step(a[..., 3:].contiguous(), done=True)
        assert torch.equal(obs, hand.see('all'))
        assert torch.equal(done, hand.done)
        if t == 0:
            assert (obs[:, :, 8] == 1).all()              # the first step after a reset is fresh for everybody
        d = done.bool()
        if d.any():                                       # auto_reset: a finished match restarts with the reset vision state
            restarted += int(d.sum())
            e = env.engine
            assert (e.neck[d][:, :22] == 0).all() and (e.view_width[d][:, :22] == 2).all() and (e.see_wait[d][:, :22] == 2).all()
            assert (obs[d][:, :, 8] == 1).all() and (obs[d][:, :, 5] == 0).all()
        rl = env.engine.reward_left
        assert torch.equal(rew[:, :11], rl[:, None].expand(n, 11)) and torch.equal(rew[:, 11:], -rl[:, None].expand(n, 11))
    assert restarted > 0
    # a masked reset resets the vision state of those matches only
    mask = torch.zeros(n, dtype=torch.uint8, device='cuda:0')
    mask[::2] = 1
    neck = env.engine.neck.clone()
    env.reset(mask)
    assert not env.engine.neck[::2].any() and torch.equal(env.engine.neck[1::2], neck[1::2])
    env.close(); hand.close()
    env = Soccer2DMatchVecEnv(64, opponent='scripted', obs='see', vision=dict(view_angle=(60.0, 90.0, 180.0)))
    assert env.reset().shape == (64, 11, 192)
    obs, rew, done, info = env.step(torch.zeros((64, 11, 5), device='cuda:0'))
    assert obs.shape == (64, 11, 192) and rew.shape == (64, 11)
    assert torch.equal(obs, env.engine.see('left'))
    with pytest.raises(ValueError):
        env.step(torch.zeros((64, 11, 3), device='cuda:0'))
    env.close()
    env = Soccer2DMatchVecEnv(64, obs='agent')            # the other observation kinds are untouched
    assert env.reset().shape == (64, 22, 224) and env.engine.vision is None
    env.close()
    env = Soccer2DMatchVecEnv(64)
    assert env.reset().shape == (64, 23, 5) and env.step(None)[0].shape == (64, 23, 5)
    env.close()


def test_engine_without_vision_is_unchanged():
    """64 cycles of the random policy with noise: an engine that never enables vision equals the CPU match oracle in every word
    after every cycle, and an engine with vision, stepped and seen alongside, keeps the same engine state"""
    from soccer2d_amd.match import MatchEngine, make_match_config
    n = 64
    kw = dict(noise=True, half_time_cycles=25, extra_half_cycles=10)
    eng = MatchEngine(n, 'cuda:0', cfg=make_match_config(**kw))
    orc = MO.MatchOracle(MO.make_match_config(noise=1, half_time_cycles=25, extra_half_cycles=10), n)
    vis = MatchEngine(n, 'cuda:0', cfg=make_match_config(**kw))
    vis.enable_vision()
    fields = MO.OBJ_FIELDS + ('catch_ban', 'card') + MO.ENV_FIELDS + ('ball_holder', 'goalie_moves', 'set_play_taker', 'last_kicker',
                                                                     'stopped_cycle', 'tick')
    for t in range(64):
        eng.step(None); orc.step(None)
        vis.step(None); vis.vision_step(done=True); vis.see('all')
        torch.cuda.synchronize()
        for f in fields:
            g, c = getattr(eng, f).cpu().numpy(), orc.get(f)
            gb = g.view(np.int32) if g.dtype == np.float32 else g
            cb = c.view(np.int32) if c.dtype == np.float32 else c
            assert np.array_equal(gb, cb), (t, f)
        assert torch.equal(eng.arena, vis.arena), t
    assert eng.vision is None
    assert list(eng.stats.cpu().numpy()) == list(orc.stats())
    eng.close(); vis.close()
