"""The audio layer on the GPU (s2d_match_hear_step, s2d_match_hear_reset): the rows and the three planes word for word the host
restatement's (tests/hear_ref.c) on played matches over consecutive steps, every hand-written scene of test_match_hear_host.py on
the device, nothing written but the four planes, every C-ABI refusal without effect, masked resets, Soccer2DMatchVecEnv(hear=True)
and an engine left bit for bit alone."""
import ctypes as C

import numpy as np
import pytest

import match_hear as H
import match_oracle as MO
import test_match_hear_host as HT
from soccer2d_amd import _capi, _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
OTHER = dict(audio_cut_dist=30.0, hear_max=3, hear_inc=1, hear_decay=2, say_msg_size=7, say_levels=9)
PLANES = ('cap_our', 'cap_opp', 'attention', 'hear')


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp('hear_ref'))


def _engine(n, hearing=None, vision=False, **kw):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(n, 'cuda:0', **kw)
    if vision:
        eng.enable_vision()
    if hearing is not None:
        eng.enable_hearing(**hearing)
    return eng


def _state(eng):
    torch.cuda.synchronize()
    s = {k: getattr(eng, k).cpu().numpy() for k in H.ENGINE_KEYS}
    s['neck'] = None if eng.vision is None else eng.neck.cpu().numpy()
    return s


def _planes(eng):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).cpu().numpy() for k in PLANES}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_planes(got, want, tag):
    for k in PLANES:
        g, w = _bits(got[k]), _bits(want[k])
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f'{tag}: {k}: {len(bad)} words differ; first at {tuple(bad[0])}: gpu={got[k][tuple(bad[0])]!r} '
                                 f'host={want[k][tuple(bad[0])]!r}')


def _random_say(rng, n, p_speak):
    a = np.zeros((n, 22, H.SAY_ROW), dtype=np.float32)
    a[..., 0] = (rng.random((n, 22)) < p_speak) * rng.choice([1.0, -3.0, 0.5], (n, 22))
    a[..., 0][rng.random((n, 22)) < 0.03] = np.nan
    cmd = rng.integers(-2, 25, (n, 22)).astype(np.float32)
    cmd[rng.random((n, 22)) < 0.6] = 0.0
    cmd[rng.random((n, 22)) < 0.03] = np.nan
    cmd[rng.random((n, 22)) < 0.03] = 2.5
    a[..., 1] = cmd
    a[..., 2:] = rng.uniform(-1.3, 1.3, (n, 22, 10))
    a[..., 2:][rng.random((n, 22, 10)) < 0.03] = np.nan
    a[..., 2:][rng.random((n, 22, 10)) < 0.03] = -0.0
    return a


@pytest.mark.parametrize('n,vision,own_stream,over', [(1, False, False, {}), (3, True, False, OTHER), (33, False, True, OTHER),
                                                      (33, True, False, {}), (515, True, True, OTHER), (515, False, False, {})])
def test_device_equals_restatement(ref, n, vision, own_stream, over):
    """40 cycles of random play, cards dealt, then for each speaker probability 8 consecutive steps (the capacities and the
    attention carry): a body step, random say rows, attention commands and done bytes, one hear step -- rows and planes equal the
    host restatement's after every step.  Some capacity and attention words start corrupt."""
    eng = _engine(n, hearing=over, vision=vision, noise=True, seed=17 + n, env_id_offset=3 * n)
    prm = H.params(seed=eng.cfg.seed, env_id_offset=eng.cfg.env_id_offset, **over)
    rng = np.random.default_rng(1000 + n)
    eng.reset()
    eng.rollout(40, with_obs=False)
    card = rng.choice([0, 1, 2], (n, 24), p=[0.8, 0.1, 0.1]).astype(np.int32)
    eng.card.copy_(torch.from_numpy(card))
    if vision:
        eng.neck.copy_(torch.from_numpy((rng.integers(-90 * 64, 90 * 64 + 1, (n, 24)) / 64.0).astype(np.float32)))
    want = _planes(eng)
    assert (want['cap_our'] == prm.hear_max).all() and (want['attention'] == -1).all()
    _assert_planes(want, H.reset_planes(n, prm), 'after enable_hearing')
    for k in ('cap_our', 'cap_opp'):                          # a few corrupt words
        want[k][rng.random((n, 24)) < 0.1] = rng.choice([-1, 99, -2 ** 31, 2 ** 31 - 1])
        getattr(eng, k).copy_(torch.from_numpy(want[k]))
    want['attention'][rng.random((n, 24)) < 0.1] = rng.choice([-2, 22, 2 ** 20])
    eng.attention.copy_(torch.from_numpy(want['attention']))
    stream = torch.cuda.Stream() if own_stream else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    heard = 0
    with torch.cuda.stream(stream):
        for p_speak in (0.0, 0.1, 1.0):
            for t in range(8):
                eng.step(None)
                say = _random_say(rng, n, p_speak)
                done = (rng.random(n) < 0.1).astype(np.uint8)
                use_say = not (p_speak == 0.0 and t % 2)      # (NULL say rows too)
                eng.hear_step(torch.from_numpy(say).cuda() if use_say else None, torch.from_numpy(done).cuda())
                want.update(H.step(ref, dict(_state(eng), **want), prm, say if use_say else None, done))
                _assert_planes(_planes(eng), want, f'n={n} p={p_speak} step {t}')
                heard += int(want['hear'][:, :, 0].sum() + want['hear'][:, :, H.REC].sum())
    torch.cuda.current_stream().wait_stream(stream)
    if n >= 33:
        assert heard > 100 and (want['hear'][:, :, 3] > 0).any() and (want['hear'][:, :, 5] > 0).any()
    eng.close()


# ---- the host scenes on the device -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene_engines():
    engs = {False: _engine(1, hearing={}), True: _engine(1, hearing={}, vision=True)}
    yield engs
    for e in engs.values():
        e.close()


def device_run(engs):
    def run(state, says, dones=None, **over):
        eng = engs[state.get('neck') is not None]
        eng.hear_params = M.hear_params(eng.lib, **over)
        for k in H.ENGINE_KEYS + PLANES + (('neck',) if eng.vision is not None else ()):
            getattr(eng, k).copy_(torch.from_numpy(np.ascontiguousarray(state[k])))
        for t, say in enumerate(says):
            eng.hear_step(None if say is None else torch.from_numpy(say).cuda(), None if dones is None else torch.from_numpy(dones[t]).cuda())
        return dict(state, **_planes(eng))
    return run


@pytest.mark.parametrize('name', sorted(HT.SCENES))
def test_scene_on_the_device(scene_engines, name):
    HT.SCENES[name](device_run(scene_engines))


def test_scene_attention_on_the_device(scene_engines, ref):
    HT.scene_attention(device_run(scene_engines), ref)


def test_scene_tie_on_the_device(scene_engines, ref):
    HT.scene_tie(device_run(scene_engines), ref)


# ---- what is written, what is refused ---------------------------------------------------------------------------------------------
def _guarded(n, rng):
    """the four planes, say, neck and done cut out of the middle of guard-filled buffers: (buffers, views)"""
    sizes = {'cap_our': n * 24, 'cap_opp': n * 24, 'attention': n * 24, 'hear': n * 22 * 32, 'say': n * 22 * 12, 'neck': n * 24}
    bufs, views = {}, {}
    for k, words in sizes.items():
        dt = torch.int32 if k in PLANES[:3] else torch.float32
        b = torch.full((words + 128,), 12345, dtype=dt, device='cuda:0')
        bufs[k], views[k] = b, b[64:64 + words]
    bufs['done'] = torch.full((n + 128,), 77, dtype=torch.uint8, device='cuda:0')
    views['done'] = bufs['done'][64:64 + n]
    views['done'].copy_(torch.from_numpy((rng.random(n) < 0.2).astype(np.uint8)))
    views['say'].copy_(torch.from_numpy(_random_say(rng, n, 0.5).reshape(-1)))
    views['neck'].copy_(torch.from_numpy(rng.integers(-90, 91, n * 24).astype(np.float32)))
    return bufs, views


def _struct(views):
    return M.S2DMatchHear(*[views[k].data_ptr() for k in PLANES])


def test_writes_only_its_planes(ref):
    n = 33
    eng = _engine(n, noise=True, seed=5)
    eng.reset()
    eng.rollout(40, with_obs=False)
    rng = np.random.default_rng(3)
    bufs, views = _guarded(n, rng)
    prm = M.hear_params(eng.lib, **OTHER)
    hs = _struct(views)
    torch.cuda.synchronize()
    arena = eng.arena.clone()
    _capi.check(eng.lib, eng.lib.s2d_match_hear_reset(eng._h, C.byref(prm), C.byref(hs), None, eng._stream()), 'reset')
    for k in PLANES[:3]:
        assert (views[k] == (-1 if k == 'attention' else 3)).all()
    inputs = {k: bufs[k].clone() for k in ('say', 'neck', 'done')}
    pads = {k: views[k].view(n, 24)[:, 22:].clone() for k in PLANES[:3]}
    for _ in range(4):
        _capi.check(eng.lib, eng.lib.s2d_match_hear_step(eng._h, C.byref(prm), C.byref(hs), views['neck'].data_ptr(), views['say'].data_ptr(),
                                                         views['done'].data_ptr(), eng._stream()), 'step')
    torch.cuda.synchronize()
    for k in PLANES:
        assert (bufs[k][:64] == 12345).all() and (bufs[k][-64:] == 12345).all(), k
    for k in ('say', 'neck', 'done'):
        assert np.array_equal(_bits(bufs[k].cpu().numpy()), _bits(inputs[k].cpu().numpy())), k    # the inputs are read only (NaNs: by bits)
    for k in PLANES[:3]:
        assert torch.equal(views[k].view(n, 24)[:, 22:], pads[k]), k   # the step leaves the two pad slots alone
    assert torch.equal(arena, eng.arena)                      # and the engine
    assert (views['hear'].view(n, 22, 32)[:, :, 0] == 1).any()
    # the same four steps (capacity 3, decay 2: heard in steps 1, 2 and 4) on the restatement
    s = {k: getattr(eng, k).cpu().numpy() for k in H.ENGINE_KEYS}
    s['neck'] = views['neck'].view(n, 24).cpu().numpy()
    hp = H.params(seed=eng.cfg.seed, env_id_offset=eng.cfg.env_id_offset, **OTHER)
    want = H.reset_planes(n, hp)
    for _ in range(4):
        want.update(H.step(ref, dict(s, **want), hp, views['say'].view(n, 22, 12).cpu().numpy(), views['done'].cpu().numpy()))
    got = {k: views[k].view(want[k].shape).cpu().numpy() for k in PLANES}
    _assert_planes(got, want, 'guarded planes')
    eng.close()


def test_refusals_leave_the_planes_unchanged():
    n = 8
    eng = _engine(n, seed=5)
    eng.reset()
    rng = np.random.default_rng(4)
    bufs, views = _guarded(n, rng)
    lib, good = eng.lib, M.hear_params(eng.lib)
    before = {k: b.clone() for k, b in bufs.items()}
    ptr = {k: v.data_ptr() for k, v in views.items()}

    def step(prm=good, neck='neck', say='say', done='done', **planes):
        p = dict(ptr, **planes)
        hs = M.S2DMatchHear(*[p[k] for k in PLANES])
        arg = [None if k is None else (p[k] if isinstance(k, str) else k) for k in (neck, say, done)]
        return lib.s2d_match_hear_step(eng._h, None if prm is None else C.byref(prm), C.byref(hs), *arg, eng._stream())

    def reset(prm=good, mask=None, **planes):
        p = dict(ptr, **planes)
        hs = M.S2DMatchHear(*[p[k] for k in PLANES])
        return lib.s2d_match_hear_reset(eng._h, None if prm is None else C.byref(prm), C.byref(hs), mask, eng._stream())

    E = _capi.S2D_EINVAL
    for field, value in HT.BAD:                               # invalid parameters
        prm = M.hear_params(lib)
        setattr(prm, field, value)
        assert step(prm=prm) == E and reset(prm=prm) == E, (field, value)
    assert step(prm=None) == E and reset(prm=None) == E
    for k in PLANES:                                          # NULL and unaligned planes
        assert step(**{k: None}) == E and reset(**{k: None}) == E, k
        assert step(**{k: ptr[k] + 2}) == E and reset(**{k: ptr[k] + 2}) == E, k
    assert step(hear=ptr['hear'] + 4) == E and reset(hear=ptr['hear'] + 8) == E      # the rows: 16 bytes
    assert step(say=ptr['say'] + 4) == E and step(say=ptr['say'] + 8) == E and step(neck=ptr['neck'] + 2) == E
    assert lib.s2d_match_hear_step(eng._h, C.byref(good), None, None, None, None, eng._stream()) == E
    assert lib.s2d_match_hear_reset(eng._h, C.byref(good), None, None, eng._stream()) == E
    # overlaps: the rows with every other plane passed, and the written planes with one another and with the inputs
    inside = ptr['hear'] + 16 * 5
    for k in PLANES[:3]:
        assert step(**{k: inside}) == E and reset(**{k: inside}) == E, k
    assert step(say=inside) == E and step(neck=inside) == E and step(done=inside) == E and reset(mask=inside) == E
    assert step(hear=ptr['say']) == E and step(hear=ptr['say'] + n * 22 * 12 * 4 - 16) == E
    assert step(cap_opp=ptr['cap_our']) == E and step(attention=ptr['cap_our'] + 4) == E and reset(cap_opp=ptr['attention']) == E
    assert step(neck=ptr['attention']) == E and step(done=ptr['cap_opp'] + 7) == E
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert np.array_equal(_bits(b.cpu().numpy()), _bits(before[k].cpu().numpy())), k
    assert step() == 0 and step(neck=None, say=None, done=None) == 0 and reset() == 0          # the good calls go through
    torch.cuda.synchronize()
    assert not torch.equal(bufs['hear'], before['hear'])   # (no NaN in the rows)
    # the Python surface
    with pytest.raises(RuntimeError):
        eng.hear_step()
    with pytest.raises(RuntimeError):
        eng.hear_rows()
    with pytest.raises(Exception):
        eng.enable_hearing(say_levels=72)
    eng.enable_hearing()
    with pytest.raises(ValueError):
        eng.hear_step(torch.zeros((n, 22, 10), device='cuda:0'))
    with pytest.raises(ValueError):
        eng.hear_step(done=torch.zeros(n + 1, dtype=torch.uint8, device='cuda:0'))
    eng.close()


def test_reset_of_a_masked_subset(ref):
    n = 37
    eng = _engine(n, hearing=OTHER, seed=9)
    eng.reset()
    eng.rollout(10, with_obs=False)
    rng = np.random.default_rng(8)
    for _ in range(3):
        eng.hear_step(torch.from_numpy(_random_say(rng, n, 0.7)).cuda())
    before = _planes(eng)
    assert (before['cap_our'][:, :22] != 3).any() and (before['hear'][:, :, 0] == 1).any()
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    eng.reset(torch.from_numpy(mask).cuda())
    after = _planes(eng)
    prm = H.params(**OTHER)
    want = H.reset(ref, dict(_state(eng), **before), prm, mask)
    _assert_planes(after, want, 'masked reset')
    m = mask.astype(bool)
    fresh = H.reset_planes(n, prm)
    for k in PLANES:
        assert np.array_equal(_bits(after[k][m]), _bits(fresh[k][m])) and np.array_equal(_bits(after[k][~m]), _bits(before[k][~m])), k
    eng.reset()
    _assert_planes(_planes(eng), fresh, 'full reset')
    eng.close()


def test_hear_rows_views_and_gathers():
    n = 5
    eng = _engine(n, hearing={})
    eng.hear.copy_(torch.arange(n * 22 * 32, device='cuda:0').view(n, 22, 32).float())
    assert eng.hear_rows() is eng.hear and eng.hear_rows('all').data_ptr() == eng.hear.data_ptr()
    assert torch.equal(eng.hear_rows('left'), eng.hear[:, :11]) and torch.equal(eng.hear_rows('right'), eng.hear[:, 11:])
    assert torch.equal(eng.hear_rows(0x200401), eng.hear[:, [0, 10, 21]])
    eng.close()


# ---- the env -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('obs,opponent', [('see', None), ('belief', None), ('see', 'scripted')])
def test_vec_env_with_hearing(ref, obs, opponent):
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    n = 48
    agents = 22 if opponent is None else 11
    slots = 'all' if opponent is None else 'left'
    env = Soccer2DMatchVecEnv(n, obs=obs, opponent=opponent, hear=True, hear_params=OTHER, noise=True, seed=31, half_time_cycles=1,
                              nr_extra_halfs=0, penalty_shoot_outs=0)
    assert env.observation_space.shape == (agents, 224) and env.action_space.shape == (agents, 17)
    e = env.engine
    prm = H.params(seed=e.cfg.seed, env_id_offset=e.cfg.env_id_offset, **OTHER)
    o = env.reset()
    assert o.shape == (n, agents, 224)
    want = H.reset_planes(n, prm)
    assert np.array_equal(_bits(o[..., 192:].cpu().numpy()), _bits(want['hear'][:, :agents]))
    rng = np.random.default_rng(12)
    finished = heard = 0
    for t in range(5):
        a = np.zeros((n, agents, 17), dtype=np.float32)
        a[..., 0] = rng.integers(0, 5, (n, agents))
        a[..., 1] = rng.uniform(-100, 100, (n, agents))
        a[..., 2] = rng.uniform(-180, 180, (n, agents))
        a[..., 3] = rng.uniform(-60, 60, (n, agents))
        a[..., 4] = rng.integers(0, 4, (n, agents))
        a[..., 5:] = _random_say(rng, n, 0.6)[:, :agents]
        o, rew, done, info = env.step(torch.from_numpy(a).cuda())
        assert o.shape == (n, agents, 224) and rew.shape == (n, agents)
        row = e.see(slots) if obs == 'see' else e.belief
        assert torch.equal(o, torch.cat([row, e.hear_rows(slots)], dim=2))      # [row | hear row], put together by hand
        say = np.zeros((n, 22, 12), dtype=np.float32)
        say[:, :agents] = a[..., 5:]
        dn = done.cpu().numpy()
        finished += int(dn.sum())
        want.update(H.step(ref, dict(_state(e), **want), prm, say, dn))
        _assert_planes(_planes(e), want, f'{obs} step {t}')
        heard += int(want['hear'][:, :, 0].sum())
    assert finished > 0 and heard > 0
    with pytest.raises(ValueError):
        env.step(torch.zeros((n, agents, 5), device='cuda:0'))
    env.close()


def test_env_without_hearing_is_unchanged():
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    env = Soccer2DMatchVecEnv(16, obs='see')
    assert env.engine.hearing is None and env.reset().shape == (16, 22, 192)
    assert env.step(torch.zeros((16, 22, 5), device='cuda:0'))[0].shape == (16, 22, 192)
    env.close()


# ---- the engine is left alone ------------------------------------------------------------------------------------------------------
def test_engine_is_left_alone():
    """33 cycles of the random policy with noise: an engine that never enables hearing equals the CPU match oracle in every word
    after every cycle, and an engine with hearing (and vision), stepped alongside with everybody speaking, keeps the same arena"""
    from soccer2d_amd.match import MatchEngine, make_match_config
    n = 64
    kw = dict(noise=True, half_time_cycles=12, extra_half_cycles=5)
    eng = MatchEngine(n, 'cuda:0', cfg=make_match_config(**kw))
    orc = MO.MatchOracle(MO.make_match_config(noise=1, half_time_cycles=12, extra_half_cycles=5), n)
    ear = MatchEngine(n, 'cuda:0', cfg=make_match_config(**kw))
    ear.enable_vision()
    ear.enable_hearing()
    fields = MO.OBJ_FIELDS + ('catch_ban', 'card') + MO.ENV_FIELDS + ('ball_holder', 'goalie_moves', 'set_play_taker', 'last_kicker',
                                                                     'stopped_cycle', 'tick')
    say = torch.from_numpy(_random_say(np.random.default_rng(2), n, 1.0)).cuda()
    for t in range(33):
        eng.step(None); orc.step(None)
        ear.step(None); ear.vision_step(done=True); ear.hear_step(say, done=True)
        torch.cuda.synchronize()
        for f in fields:
            g, c = getattr(eng, f).cpu().numpy(), orc.get(f)
            assert np.array_equal(_bits(g), _bits(c)), (t, f)
        assert torch.equal(eng.arena, ear.arena), t
    assert eng.hearing is None and (ear.hear[:, :, 0] == 1).any()
    eng.close(); ear.close()


# ---- the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('obs', ['see', 'belief'])
def test_ppo_example_with_hear(obs):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gym-soccer-2d-env_amd', 'examples'))
    try:
        import ppo_match_selfplay as ex
    finally:
        sys.path.pop(0)
    stats = ex.main(['--hear', '--obs', obs, '--num-matches', '8', '--steps', '6', '--iterations', '2', '--epochs', '1', '--minibatches', '2'])
    assert len(stats) == 2
    for key in ('policy_loss', 'value_loss', 'entropy', 'approx_kl', 'mean_reward', 'heard_share'):
        assert np.isfinite(stats[-1][key]), (key, stats[-1])
    assert stats[-1]['heard_share'] > 0.5                     # everybody speaks every cycle: nearly every listener hears a teammate
    for bad in (['--hear'], ['--hear', '--obs', 'see', '--fused-learner'], ['--hear', '--obs', 'see', '--shaping', 'goal=1']):
        with pytest.raises(SystemExit):
            ex.main(bad)
