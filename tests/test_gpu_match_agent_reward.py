"""The agent reward on the GPU (s2d_match_set_agent_reward / s2d_match_rollout_reward): bit-exact to the host restatement
(tests/agent_reward_ref.c) cycle by cycle for every kernel family that carries it, one T-cycle launch equal to T one-cycle
launches, no interference with any other record or with the state, weights read when the kernel runs (graph replay included),
goal-only weights equal to the signed team reward, the refusals, and Soccer2DMatchVecEnv(reward=...).

Shapes: a workgroup holds 8 matches and a wave 2, so N in {1, 7, 9, 521} (a lone match, a partial workgroup, one match past a
workgroup, many workgroups with a partial last one) and T in {1, 2, 33}."""
import ctypes as C

import numpy as np
import pytest

import agent_obs as A
import agent_reward as R
from soccer2d_amd import _capi_match as M
from test_gpu_match_policy import _policy, _qnet

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
W = R.WEIGHTS
SIGN = np.array([1.0] * 11 + [-1.0] * 11, dtype=np.float32)
HETERO = dict(hetero_seed=3, player_type_id=[0] + list(range(1, 11)) + [0] + [11, 12, 13, 14, 15, 16, 17, 1, 2, 3],
              kickable_margin=0.8, server_params={'ball_decay': 0.9, 'player_speed_max': 1.2})


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return R.Ref(tmp_path_factory.mktemp('agent_reward'))


def _setup_random(eng):
    return {}


def _setup_scripted(eng):
    eng.set_controllers({'left': 'scripted', 'right': 'scripted'})
    return {}


def _setup_general(eng):
    eng.set_controllers({'left': 'scripted', 'right': 'random'})
    assert 'general' in eng.kernel_name()
    return dict(record_actions=True)


def _setup_two_nets(eng):
    eng.set_network(_qnet(32, 16, 7, 0.25, 5), 'left')
    eng.set_opponent_network(_qnet(16, 32, 5, 0.25, 6), 'right')
    return dict(net_index=True)


def _setup_policy(eng):
    eng.set_network(_policy(32, 32, 6, 'tanh', 41), 'all')
    return dict(net_index=True, logp=True, agent_obs='all')


CASES = {'random_noise': (dict(), _setup_random), 'scripted': (dict(seed=5), _setup_scripted),
         'general_hetero': (HETERO, _setup_general), 'two_networks': (dict(seed=7), _setup_two_nets),
         'policy': (dict(seed=9), _setup_policy)}
RECORDS = ('obs', 'reward', 'mode', 'done', 'actions', 'net_index', 'logp', 'agent_obs', 'agent_reward')


def _engine(n, case='random_noise', weights=W, chaser_only=False, scene=True, **kw):
    """an engine of `case` with short periods, noise on, the scenes written over its reset state, and (weights not None) the
    agent reward set; returns (engine, the case's rollout keywords)"""
    from soccer2d_amd.match import MatchEngine
    ckw, setup = CASES[case]
    eng = MatchEngine(n, 'cuda:0', noise=True, **{**R.SHORT, **ckw, **kw})
    rkw = setup(eng)
    eng._actors = (eng.network, eng.opponent_network)
    eng.reset()
    if scene:
        _write(eng, R.write_scene(_state(eng), seed=n))
    if weights is not None:
        eng.set_agent_reward(weights, chaser_only)
    return eng, rkw


def _state(eng):
    return {k: getattr(eng, k).cpu().numpy() for k in A.OBJ_PLANES + A.ENV_WORDS}


def _full_state(eng):
    return {name: getattr(eng, name).cpu().numpy() for name, _t, _d, trail in M.MATCH_BUFFER_FIELDS if trail is not None}


def _write(eng, s):
    for k in A.OBJ_PLANES + A.ENV_WORDS:
        getattr(eng, k).copy_(torch.from_numpy(np.ascontiguousarray(s[k])))


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, 'cpu') else a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, tag):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f'{tag}: {len(bad)} of {a.size} words differ; first at {tuple(bad[0])}: '
                             f'{a[tuple(bad[0])]:#x} vs {b[tuple(bad[0])]:#x}')


def _same_records(a, b, tag, skip=()):
    for k in RECORDS:
        if k in skip or (a.get(k) is None and b.get(k) is None):
            continue
        _same(a[k], b[k], f'{tag}: {k}')


def _same_state(a, b, tag):
    sa, sb = _full_state(a), _full_state(b)
    for k in sa:
        _same(sa[k], sb[k], f'{tag}: state {k}')


def _cycle_by_cycle(ref, case, n, chaser_only, T=33):
    """T one-cycle launches, each compared with the restatement of (S, S'); returns the stacked records, the summed |w * term|
    per term and the number of done cycles"""
    eng, rkw = _engine(n, case, chaser_only=chaser_only)
    assert eng.kernel_name().endswith(', agent reward>')
    prm = A.params(eng.cfg)
    w = np.array(W, dtype=np.float32)
    contrib, dones, steps = np.zeros(6), 0, []
    s0 = _state(eng)
    for t in range(T):
        out = eng.rollout(1, agent_reward=True, **rkw)
        torch.cuda.synchronize()
        s1 = _state(eng)
        want, terms = ref.reward(prm, s0, s1, eng.reward_left.cpu().numpy(), w, chaser_only)
        _same(out['agent_reward'][0], want, f'{case} n={n} chaser_only={chaser_only} cycle {t}')
        contrib += np.abs(terms.astype(np.float64) * w).sum(axis=(0, 1))
        dones += int(out['done'].sum())
        steps.append({k: v.clone() for k, v in out.items() if v is not None})
        s0 = s1
    return eng, rkw, steps, contrib, dones


@pytest.mark.parametrize('chaser_only', [False, True])
@pytest.mark.parametrize('case,n', [(c, 521) for c in sorted(CASES)] + [('random_noise', k) for k in (1, 7, 9)])
def test_bit_exact_to_the_restatement_cycle_by_cycle(ref, case, n, chaser_only):
    eng, _rkw, _steps, contrib, dones = _cycle_by_cycle(ref, case, n, chaser_only)
    print(f'{case} n={n} chaser_only={chaser_only}: sum |w term| per term {contrib}, done cycles {dones}')
    if n >= 7:                       # (a lone match is one scene: it cannot show every term)
        assert (contrib > 0).all() and dones >= 1, (contrib, dones)
    eng.close()


@pytest.mark.parametrize('case', ['general_hetero', 'policy'])
def test_one_launch_equals_the_one_cycle_launches(ref, case):
    n, T = 9, 33
    eng, rkw, steps, _c, _d = _cycle_by_cycle(ref, case, n, True, T)
    one, _ = _engine(n, case, chaser_only=True)
    out = one.rollout(T, agent_reward=True, **rkw)
    torch.cuda.synchronize()
    for k in RECORDS:
        if out.get(k) is not None:
            _same(out[k], torch.cat([s[k] for s in steps]), f'{case}: {k}')
    _same_state(one, eng, case)
    eng.close(); one.close()


@pytest.mark.parametrize('T', [1, 2, 33])
@pytest.mark.parametrize('n', [1, 7, 9, 521])
@pytest.mark.parametrize('case', ['random_noise', 'two_networks', 'policy'])
def test_no_interference_with_the_other_records_and_the_state(case, n, T):
    kw = dict(record_actions=True, net_index=True, logp=True, agent_obs='left') if case != 'random_noise' else dict(record_actions=True)
    plain, _ = _engine(n, case, weights=None)
    name = plain.kernel_name()
    a = plain.rollout(T, **kw)
    withr, _ = _engine(n, case, chaser_only=True)
    assert withr.kernel_name() == name[:-1] + ', agent reward>'
    b = withr.rollout(T, agent_reward=True, **kw)
    unasked, _ = _engine(n, case)                       # a reward set, no record asked for: the launch without it
    c = unasked.rollout(T, **kw)
    torch.cuda.synchronize()
    assert 'agent_reward' not in a and 'agent_reward' not in c and tuple(b['agent_reward'].shape) == (T, n, 22)
    _same_records(a, b, f'{case} n={n} T={T}', skip=('agent_reward',))
    _same_records(a, c, f'{case} n={n} T={T} (no record)')
    _same_state(plain, withr, f'{case} n={n} T={T}')
    _same_state(plain, unasked, f'{case} n={n} T={T} (no record)')
    withr.set_agent_reward(None)
    assert withr.kernel_name() == name
    for e in (plain, withr, unasked):
        e.close()


def test_kernel_names_without_a_reward_are_the_existing_literals():
    from soccer2d_amd.match import MatchEngine
    want = {(): 's2d_match_rollout_kernel<stock rules, own schedule>', ('ctl',): 's2d_match_rollout_kernel<stock rules, own schedule, controllers>',
            ('net',): 's2d_match_rollout_kernel<stock rules, own schedule, network>',
            ('net', 'opp'): 's2d_match_rollout_kernel<stock rules, own schedule, two networks>',
            ('pol',): 's2d_match_rollout_kernel<stock rules, own schedule, policy network>'}
    for what, name in want.items():
        eng = MatchEngine(3, 'cuda:0', **R.SHORT)
        if 'ctl' in what:
            eng.set_controllers({'left': 'scripted', 'right': 'random'})
        if 'net' in what:
            eng.set_network(_qnet(16, 16, 4, 0.1, 1), 'left')
        if 'opp' in what:
            eng.set_opponent_network(_qnet(16, 16, 4, 0.1, 2), 'right')
        if 'pol' in what:
            eng.set_network(_policy(16, 16, 4, 'tanh', 3), 'left')
        assert eng.kernel_name() == name
        eng.set_agent_reward(W)
        assert eng.kernel_name() == name[:-1] + ', agent reward>'
        eng.close()
    eng = MatchEngine(3, 'cuda:0')
    assert eng.kernel_name() == 's2d_match_rollout_kernel<stock, stock types>'
    eng.close()


def test_weights_are_read_when_the_kernel_runs():
    n, T = 9, 2
    w2 = (0.5, 0.07, 0.3, 0.9, 0.13, 0.21)
    first, _ = _engine(n, 'scripted', weights=W)
    second, _ = _engine(n, 'scripted', weights=w2)
    a, b = first.rollout(T, agent_reward=True)['agent_reward'].clone(), second.rollout(T, agent_reward=True)['agent_reward'].clone()
    assert not torch.equal(a, b)
    # in place, between two launches
    eng, _ = _engine(n, 'scripted', weights=W)
    eng.agent_reward_weights.copy_(torch.tensor(w2, device='cuda:0'))
    _same(eng.rollout(T, agent_reward=True)['agent_reward'], b, 'weights written in place')
    # ... and under a single-stream graph replay
    eng, _ = _engine(n, 'scripted', weights=W)
    start = _state(eng)
    out = eng.alloc_rollout(T, with_obs=False)
    out['agent_reward'] = torch.zeros((T, n, 22), dtype=torch.float32, device='cuda:0')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.rollout(T, out=out, agent_reward=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.rollout(T, out=out, agent_reward=True)
    for w, want in ((W, a), (w2, b)):
        eng.reset()
        _write(eng, start)
        eng.agent_reward_weights.copy_(torch.tensor(w, device='cuda:0'))
        g.replay()
        torch.cuda.synchronize()
        _same(out['agent_reward'], want, f'graph replay with weights {w}')


@pytest.mark.parametrize('case', ['random_noise', 'policy'])
def test_goal_only_weights_give_the_signed_team_reward(case):
    eng, rkw = _engine(521, case, weights={'goal': 1.0})
    out = eng.rollout(33, agent_reward=True, **rkw)
    torch.cuda.synchronize()
    r = out['reward'].cpu().numpy()
    assert np.count_nonzero(r > 0) and np.count_nonzero(r < 0)
    assert np.array_equal(out['agent_reward'].cpu().numpy(), r[:, :, None] * SIGN)      # values: -0.0 == 0.0
    eng.close()


def test_refusals_leave_the_engine_as_it_was():
    n, T = 7, 2
    eng, _ = _engine(n, 'scripted')
    twin, _ = _engine(n, 'scripted')
    lib, h = eng.lib, eng._h
    w = eng.agent_reward_weights
    bad = [M.S2DMatchAgentReward(None, 0), M.S2DMatchAgentReward(w.data_ptr() + 2, 0), M.S2DMatchAgentReward(w.data_ptr(), 2),
           M.S2DMatchAgentReward(w.data_ptr(), -1)]
    for rw in bad:
        assert lib.s2d_match_set_agent_reward(h, C.byref(rw)) == -1
    assert eng.kernel_name().endswith(', agent reward>')
    # a see network beside an agent reward, from either setter
    from soccer2d_amd.actor import MatchQNetActor
    see = MatchQNetActor(16, 16, 3, epsilon=0.0, obs='see')
    eng.enable_vision()
    with pytest.raises(Exception, match='agent reward'):
        eng.set_network(see, 'left')
    with pytest.raises(ValueError, match='see'):
        eng.rollout(T, agent_reward=True, see_obs='all')
    other, _ = _engine(n, 'scripted', weights=None)
    other.enable_vision()
    other.set_controllers(None)
    other.set_network(see, 'left')
    rw = M.S2DMatchAgentReward(w.data_ptr(), 0)
    assert other.lib.s2d_match_set_agent_reward(other._h, C.byref(rw)) == -1
    assert other.kernel_name().endswith('see network>')
    other.set_network(None)
    # a record while no reward is set; an unaligned record
    buf = torch.zeros(T * n * 22 + 1, dtype=torch.float32, device='cuda:0')
    ro = M.S2DMatchRollout()
    st = eng._stream()
    assert other.lib.s2d_match_rollout_reward(other._h, T, None, C.byref(ro), None, None, None, 0, None, C.c_void_p(buf.data_ptr()), st) == -1
    assert lib.s2d_match_rollout_reward(h, T, None, C.byref(ro), None, None, None, 0, None, C.c_void_p(buf.data_ptr() + 2), st) == -1
    with pytest.raises(ValueError, match='set_agent_reward'):
        other.rollout(T, agent_reward=True)
    # after all of it the engine launches what its twin launches
    a, b = eng.rollout(T, agent_reward=True), twin.rollout(T, agent_reward=True)
    torch.cuda.synchronize()
    _same_records(a, b, 'after the refusals')
    _same_state(eng, twin, 'after the refusals')
    # with no record the entry point is s2d_match_rollout_policy
    assert lib.s2d_match_rollout_reward(h, T, None, C.byref(ro), None, None, None, 0, None, None, st) == 0
    twin.rollout(T, with_obs=False)
    torch.cuda.synchronize()
    _same_state(eng, twin, 'no record')
    for e in (eng, twin, other):
        e.close()


@pytest.mark.parametrize('opponent', [None, 'scripted'])
def test_vecenv_returns_the_record(opponent):
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    n, agents = 9, 22 if opponent is None else 11
    kw = dict(noise=True, **R.SHORT)
    env = Soccer2DMatchVecEnv(n, 'cuda:0', opponent=opponent, obs='agent', reward=dict(zip(M.REWARD_TERMS, W)), chaser_only=True, **kw)
    plain = Soccer2DMatchVecEnv(n, 'cuda:0', opponent=opponent, obs='agent', **kw)
    eng, _ = _engine(n, 'random_noise', chaser_only=True, scene=False)
    if opponent is not None:
        eng.set_controllers({'left': 'external', 'right': opponent})
    envs = (env, plain)
    for v in envs:
        v.reset()
        _write(v.engine, R.write_scene(_state(v.engine), seed=n))
    _write(eng, R.write_scene(_state(eng), seed=n))
    rng = np.random.default_rng(2)
    for t in range(6):
        act = np.stack([rng.integers(1, 4, (n, agents)), rng.uniform(0, 100, (n, agents)), rng.uniform(-90, 90, (n, agents))],
                       axis=2).astype(np.float32)
        full = np.zeros((1, n, 22, 3), dtype=np.float32)
        full[0, :, :agents] = act
        obs, rew, done, _info = env.step(torch.from_numpy(act).cuda())
        pobs, prew, pdone, _pinfo = plain.step(torch.from_numpy(act).cuda())
        want = eng.rollout(1, actions=torch.from_numpy(full).cuda(), agent_reward=True)
        torch.cuda.synchronize()
        assert tuple(rew.shape) == (n, agents)
        _same(rew, want['agent_reward'][0, :, :agents], f'shaped reward, step {t}')
        _same(obs, pobs, f'obs, step {t}'); _same(done, pdone, f'done, step {t}')
        _same(prew, plain.engine.reward_left[:, None] * torch.tensor(SIGN[:agents], device='cuda:0'), f'default reward, step {t}')
    assert plain.engine.kernel_name().endswith('>') and 'agent reward' not in plain.engine.kernel_name()
    with pytest.raises(ValueError):
        Soccer2DMatchVecEnv(n, 'cuda:0', obs='state', reward=W)
    with pytest.raises(ValueError):
        Soccer2DMatchVecEnv(n, 'cuda:0', obs='agent', reward='dense')
    for v in envs:
        v.close()
    eng.close()
