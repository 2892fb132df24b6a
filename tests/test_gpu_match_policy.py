"""11v11 policy slots (s2d_match_set_policy_network, s2d_match_rollout_policy): every policy slot takes, bit for bit and with
noise on, the index the host restatement (tests/match_policy_ref.c on tests/agent_obs_ref.c's rows) takes and records its
log-probability -- in closed loop against the CPU oracle, over slot masks, widths, K and activations that reach every path, in
every combination of kinds across the two roles, under graph replay with the deterministic word switched; the records, the
regression guard without a policy network, the rejections, and the layers above (league, vec env, the PPO example)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import agent_obs as A
import match_net as MN
import match_policy as MP
from test_gpu_match import _pair, assert_match_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
ALL, LEFT, RIGHT = 0x3FFFFF, 0x7FF, 0x3FF800
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('match_policy')
    return MP.build(d), MN.build(d), A.build(d)


def _module(h1, h2, k, seed, act):
    torch.manual_seed(seed)
    f = torch.nn.Tanh if act == 'tanh' else torch.nn.ReLU
    m = torch.nn.Sequential(torch.nn.Linear(224, h1), f(), torch.nn.Linear(h1, h2), f(), torch.nn.Linear(h2, k))
    with torch.no_grad():
        m[4].weight.mul_(4.0)                              # logits a few units apart: neither uniform nor one-hot
    return m.to('cuda:0')


def _table(k, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(1, 6, k).astype(np.float32), rng.uniform(-100, 100, k).astype(np.float32),
                     rng.uniform(-180, 180, k).astype(np.float32)], axis=1)


def _policy(h1, h2, k, act, seed, det=False):
    from soccer2d_amd.actor import MatchPolicyActor
    return MatchPolicyActor.from_module(_module(h1, h2, k, seed, act), _table(k, 1000 + seed), deterministic=det)


def _qnet(h1, h2, k, eps, seed):
    from soccer2d_amd.actor import MatchQNetActor
    return MatchQNetActor.from_module(_module(h1, h2, k, seed, 'relu'), _table(k, 1000 + seed), epsilon=eps)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, tag):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (tag, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f'{tag}: {len(bad)} entries differ; first at {i}: gpu={got[i]!r} host={want[i]!r}')


def _slots(mask):
    return [i for i in range(22) if (mask >> i) & 1]


def _host(actor):
    """what the host restatement needs of an actor, as it is now"""
    d = dict(params=actor.params.cpu().numpy(), table=actor.table.cpu().numpy(), h1=actor.hidden1, h2=actor.hidden2,
             k=actor.n_actions, policy=getattr(actor, 'kind', 'qnet') == 'policy')
    if d['policy']:
        d.update(act=1 if actor.activation == 'tanh' else 0, det=int(actor.deterministic_tensor.item()))
    else:
        d.update(eps=actor.epsilon)
    return d


def _want(refs, rows, net, seed, gid, tick, slots):
    """(index, logp) of the slots of one network on their rows [N, len(slots), 224]"""
    PL, L, _ = refs
    if net['policy']:
        return MP.actions(PL, rows, net['params'], net['h1'], net['h2'], net['k'], net['act'], net['det'], seed, gid, tick, slots)
    idx = MN.indices(L, rows, net['params'], net['h1'], net['h2'], net['k'], net['eps'], seed, gid, tick, slots)
    return idx, np.zeros(idx.shape, dtype=np.float32)


def _engine_pair(n, general, monkeypatch):
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    return _pair(n, noise=True, seed=23 if general else 0x5EED)


def _install(eng, a, mask_a, b=None, mask_b=0, swap=False):
    if swap:
        eng.set_network(b, mask_b)
        eng.set_opponent_network(a, mask_a)
    else:
        eng.set_network(a, mask_a)
        if b is not None:
            eng.set_opponent_network(b, mask_b)


def _closed_loop(refs, n, T, a, mask_a, b, mask_b, obs_mask, general, monkeypatch, launches=1, swap=False):
    """launches x T cycles; per cycle: recorded rows == host rows of the oracle state; index and logp of every network slot ==
    the host's under its own network; logp 0 and index -1 elsewhere; recorded actions == the table's row; the oracle driven by
    the recorded actions ends where the engine does.  Returns the records of the last launch."""
    AL = refs[2]
    eng, orc = _engine_pair(n, general, monkeypatch)
    _install(eng, a, mask_a, b, mask_b, swap)
    name = eng.kernel_name()
    assert name.endswith('two networks, policy>' if b is not None else 'policy network>') and ('general' in name) == general, name
    eng.reset(); orc.reset()
    prm = A.params(eng.cfg)
    nets = [(_host(a), _slots(mask_a), 'A')] + ([(_host(b), _slots(mask_b), 'B')] if b is not None else [])
    others = [i for i in range(22) if not ((mask_a | mask_b) >> i) & 1]
    gid = np.arange(n) + eng.cfg.env_id_offset
    keep = None
    for launch in range(launches):
        out = eng.rollout(T, record_actions=True, net_index=True, agent_obs=obs_mask, with_obs=False, logp=True)
        rec, idx, lp, aobs = (out[k].cpu().numpy() for k in ('actions', 'net_index', 'logp', 'agent_obs'))
        for t in range(T):
            s = {k: orc.get(k) for k in A.OBJ_PLANES + A.ENV_WORDS}
            tag = f'launch {launch} t={t}'
            _same(aobs[t], A.observations(AL, s, prm, obs_mask), f'agent_obs {tag}')
            for net, slots, who in nets:
                mask = sum(1 << i for i in slots)
                wi, wl = _want(refs, A.observations(AL, s, prm, mask), net, eng.cfg.seed, gid, orc.get('tick'), slots)
                _same(idx[t][:, slots], wi, f'net_index of {who} {tag}')
                _same(lp[t][:, slots], wl, f'logp of {who} {tag}')
                _same(rec[t][:, slots], net['table'][idx[t][:, slots]], f'actions of {who} {tag}')
            assert (idx[t][:, others] == -1).all() and (_bits(lp[t][:, others]) == 0).all()
            orc.step(rec[t])
        keep = dict(idx=idx, lp=lp, rec=rec, aobs=aobs, arena=eng.arena.clone())
    assert_match_same(eng, orc, 'end state')
    eng.close()
    return keep


@pytest.mark.parametrize('general', [False, True])
def test_closed_loop_three_matches_two_launches(refs, general, monkeypatch):
    """3 matches (the second wave has one empty half) x 6 cycles x 2 launches, a 32-48-6 tanh policy on all 22 slots"""
    out = _closed_loop(refs, 3, 6, _policy(32, 48, 6, 'tanh', 3), ALL, None, 0, ALL, general, monkeypatch, launches=2)
    assert len(np.unique(out['idx'])) > 3 and (out['lp'] < 0).all()      # sampled: not one index, real log-probabilities


# masks: one slot; 8 slots = a full tile; 9 = one row into the second tile; all 22.  Every mask, width pair, K and activation
# meets each kernel family at least once.
ONE, EIGHT, NINE = 1 << 13, 0xFF, 0x1FF << 6
GRID = [
    # mask, widths, K, activation, general
    (ONE,   (16, 16), 1,  'relu', False), (ONE,   (64, 64), 64, 'tanh', True),
    (EIGHT, (64, 64), 16, 'tanh', False), (EIGHT, (16, 16), 17, 'relu', True),
    (NINE,  (16, 16), 17, 'tanh', False), (NINE,  (64, 64), 1,  'relu', True),
    (ALL,   (64, 64), 64, 'relu', False), (ALL,   (16, 16), 16, 'tanh', True),
]


@pytest.mark.parametrize('mask,widths,k,act,general', GRID)
def test_shape_grid(refs, mask, widths, k, act, general, monkeypatch):
    _closed_loop(refs, 3, 3, _policy(widths[0], widths[1], k, act, 7 + k), mask, None, 0, mask | 1, general, monkeypatch)


def _roles(case):
    if case == 'policy + qnet':
        return _policy(32, 32, 7, 'tanh', 11), LEFT, _qnet(48, 16, 9, 0.5, 12), RIGHT
    if case == 'policy + policy':
        return _policy(16, 48, 5, 'tanh', 13), LEFT, _policy(64, 32, 33, 'relu', 14), RIGHT
    if case == 'qnet + policy':
        return _qnet(32, 32, 7, 0.5, 15), LEFT, _policy(48, 16, 9, 'relu', 16), RIGHT
    if case == 'widest pair':
        return _policy(64, 64, 64, 'tanh', 17), LEFT, _policy(64, 64, 64, 'relu', 18), RIGHT
    assert case == 'straddle 5 + 6'                        # 5 rows of A and 6 of B: one tile in slot order would mix them
    return _policy(32, 32, 7, 'relu', 19), 0x1F << 2, _qnet(16, 16, 4, 0.5, 20), 0x3F << 12


@pytest.mark.parametrize('case,general', [('policy + qnet', False), ('policy + policy', True), ('qnet + policy', False),
                                          ('widest pair', False), ('widest pair', True),     # staged / the unstaged fallback
                                          ('straddle 5 + 6', True)])
def test_role_combinations_and_swap_symmetry(refs, case, general, monkeypatch):
    """3 matches x 4 cycles against the reference, and (A in role 0, B in role 1) == (B in role 0, A in role 1) bitwise"""
    a, ma, b, mb = _roles(case)
    x = _closed_loop(refs, 3, 4, a, ma, b, mb, ma | mb, general, monkeypatch)
    y = _closed_loop(refs, 3, 4, a, ma, b, mb, ma | mb, general, monkeypatch, swap=True)
    for k in ('idx', 'lp', 'rec', 'aobs'):
        _same(x[k], y[k], f'swap symmetry: {k}')
    assert torch.equal(x['arena'], y['arena'])


def _fresh(n):
    from soccer2d_amd.match import MatchEngine
    return MatchEngine(n, 'cuda:0', noise=True)


def test_deterministic_switch_under_graph_replay(refs):
    """one captured launch, replayed with the word at 0, then at 1 with new weights and a new table: each replay is the
    reference's for what the buffers held"""
    n, T = 3, 4
    a = _policy(32, 32, 6, 'tanh', 41)
    eng = _fresh(n)
    eng.set_network(a, 'all')
    eng.reset()
    out = eng.alloc_rollout(T, with_obs=False, record_actions=True)
    kw = dict(out=out, record_actions=True, net_index=True, agent_obs='all', with_obs=False, logp=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.rollout(T, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.rollout(T, **kw)
    gid = np.arange(n) + eng.cfg.env_id_offset
    slots = _slots(ALL)

    def replay(tag):
        eng.reset()
        tick0 = eng.tick.cpu().numpy().astype(np.int64)
        g.replay()
        torch.cuda.synchronize()
        rows, idx, lp, rec = (out[k].cpu().numpy() for k in ('agent_obs', 'net_index', 'logp', 'actions'))
        net = _host(a)
        for t in range(T):
            wi, wl = _want(refs, rows[t], net, eng.cfg.seed, gid, tick0 + t, slots)
            _same(idx[t], wi, f'{tag} index t={t}')
            _same(lp[t], wl, f'{tag} logp t={t}')
            _same(rec[t], net['table'][idx[t]], f'{tag} actions t={t}')
        return rows, idx

    replay('sampling')
    with torch.no_grad():
        for p in a._module.parameters():
            p.add_(torch.randn_like(p) * 0.5)
    a.sync()
    a.set_table(_table(6, 99))
    a.deterministic = True
    rows, idx = replay('deterministic, new weights and table')
    y = MP.forward(refs[0], rows[0], a.params.cpu().numpy(), 32, 32, 6, 1)
    _same(idx[0], y.argmax(axis=-1).astype(np.int32), 'greedy: the first maximum')
    eng.close()


def _run(eng, T, **kw):
    eng.reset()
    out = eng.rollout(T, record_actions=True, net_index=True, agent_obs='all', with_obs=False, **kw)
    torch.cuda.synchronize()
    return out


def test_logp_buffer_and_the_net_entry_point():
    """logp is exactly 0.0f on the slots of no network and of the Q-network; s2d_match_rollout_net with a policy network set
    takes the same indices to the same state"""
    n, T = 3, 4
    p, q = _policy(32, 16, 5, 'tanh', 51), _qnet(16, 32, 7, 0.5, 52)
    x, y = _fresh(n), _fresh(n)
    for e in (x, y):
        e.set_network(p, 0x3F)                             # slots 0..5 on the policy, 11..16 on the Q-network, the rest random
        e.set_opponent_network(q, 0x3F << 11)
    ox = _run(x, T, logp=True)
    lp = ox['logp'].cpu().numpy()
    assert (lp[..., :6] < 0).all() and np.isfinite(lp).all()
    assert (_bits(lp[..., 6:]) == 0).all()                 # +0.0f, bit for bit
    oy = _run(y, T)
    assert 'logp' not in oy
    for k in ('net_index', 'actions', 'agent_obs', 'reward', 'mode', 'done'):
        assert torch.equal(ox[k], oy[k]), k
    assert torch.equal(x.arena, y.arena)
    x.close(); y.close()


def test_without_a_policy_network_it_is_rollout_net():
    """the regression guard: Q-networks only (and no network at all) -- s2d_match_rollout_policy == s2d_match_rollout_net
    bitwise, logp all zero, and the kernel is the one it was"""
    n, T = 3, 4
    a, b = _qnet(32, 16, 5, 0.3, 61), _qnet(16, 32, 7, 0.1, 62)
    for two in (True, False, None):
        x, y = _fresh(n), _fresh(n)
        for e in (x, y):
            if two is not None:
                e.set_network(a, 'left')
            if two:
                e.set_opponent_network(b, 'right')
        assert 'policy' not in x.kernel_name()
        ox = x.alloc_rollout(T, with_obs=False, record_actions=True)
        ox['logp'] = torch.full((T, n, 22), 7.0, device='cuda:0')        # (a stale buffer is overwritten)
        x.reset()
        ox = x.rollout(T, out=ox, record_actions=True, net_index=True, agent_obs='all', with_obs=False, logp=True)
        oy = _run(y, T)
        torch.cuda.synchronize()
        assert (_bits(ox['logp'].cpu().numpy()) == 0).all()
        for k in ('net_index', 'actions', 'agent_obs', 'reward', 'mode', 'done'):
            assert torch.equal(ox[k], oy[k]), (two, k)
        x.close(); y.close()


def test_rejections_leave_the_engine_unchanged():
    from soccer2d_amd import _capi_match as M
    from soccer2d_amd.actor import MatchQNetActor
    n, T = 3, 3
    a, b = _policy(32, 32, 8, 'tanh', 71), _qnet(16, 48, 5, 0.1, 72)
    eng, twin = _fresh(n), _fresh(n)
    for e in (eng, twin):
        e.set_network(a, 'left')
        e.set_opponent_network(b, 'right')
        e.reset()
    lib, h = eng.lib, eng._h
    good = a.c_struct(LEFT)
    cases = [('h1', 24), ('h2', 80), ('n_actions', 0), ('n_actions', 65), ('slot_mask', 0), ('slot_mask', 1 << 22),
             ('activation', 2), ('activation', -1), ('params', a.params.data_ptr() + 4), ('params', None),
             ('deterministic', None), ('deterministic', a.deterministic_tensor.data_ptr() + 2),
             ('table', a.table.data_ptr() + 2), ('table', None),
             ('slot_mask', LEFT | (1 << 11)), ('slot_mask', 1 << 21), ('slot_mask', ALL)]          # overlap role 1's mask
    for field, value in cases:
        s = M.S2DMatchPolicyNet.from_buffer_copy(good)
        setattr(s, field, value)
        assert lib.s2d_match_set_policy_network(h, 0, C.byref(s)) == -1, (field, value)
        assert lib.s2d_last_error()
    for role in (-1, 2):
        assert lib.s2d_match_set_policy_network(h, role, C.byref(good)) == -1 and b'role' in lib.s2d_last_error()
    assert lib.s2d_match_set_policy_network(h, 1, C.byref(a.c_struct(RIGHT | 1))) == -1      # role 1 against role 0's mask
    assert lib.s2d_match_set_network(h, C.byref(b.c_struct(ALL))) == -1                      # a Q-network against the other role
    lp = torch.zeros((T, n, 22), device='cuda:0')
    assert lib.s2d_match_rollout_policy(h, T, None, None, None, None, C.c_void_p(lp.data_ptr() + 2), 0, None, None) == -1
    assert b'logp' in lib.s2d_last_error()
    with pytest.raises(ValueError):
        eng.set_network(a, 'all')
    assert eng.kernel_name().endswith('two networks, policy>') and eng.kernel_name() == twin.kernel_name()
    kw = dict(record_actions=True, net_index=True, agent_obs='all', with_obs=False, logp=True)
    ox, oy = eng.rollout(T, **kw), twin.rollout(T, **kw)
    torch.cuda.synchronize()
    for k in ('net_index', 'logp', 'actions', 'agent_obs'):
        assert torch.equal(ox[k], oy[k]), k
    assert torch.equal(eng.arena, twin.arena)
    # roles hold one network of either kind; NULL clears whatever is there
    assert lib.s2d_match_set_network(h, None) == 0                                           # clears the policy in role 0
    assert eng.kernel_name().endswith('network>') and 'policy' not in eng.kernel_name()
    assert lib.s2d_match_set_policy_network(h, 1, C.byref(a.c_struct(RIGHT))) == 0           # replaces the Q-network in role 1
    assert eng.kernel_name().endswith('policy network>')
    assert lib.s2d_match_set_opponent_network(h, None) == 0
    assert not eng.kernel_name().endswith('network>')
    assert lib.s2d_match_set_policy_network(h, 0, C.byref(good)) == 0 and lib.s2d_match_set_policy_network(h, 0, None) == 0
    assert not eng.kernel_name().endswith('network>')
    # the see network: role 0 clears it, role 1 beside it is refused, and it clears policy networks
    eng.network = eng.opponent_network = None
    eng.network_mask = eng.opponent_mask = 0
    eng.enable_vision()
    see = MatchQNetActor(16, 16, 3, epsilon=0.0, obs='see')
    eng.set_opponent_network(a, 'right')
    eng.set_network(see, 'left')
    assert eng.kernel_name().endswith('see network>')
    assert lib.s2d_match_set_policy_network(h, 1, C.byref(a.c_struct(RIGHT))) == -1 and b'see network' in lib.s2d_last_error()
    assert lib.s2d_match_set_policy_network(h, 0, C.byref(good)) == 0
    assert eng.kernel_name().endswith('policy network>')
    eng.close(); twin.close()


def test_league_play_networks_with_a_policy_actor():
    from soccer2d_amd import league
    n, T = 4, 8
    learner, frozen = _policy(32, 32, 8, 'tanh', 81), _qnet(16, 16, 4, 0.1, 82)
    eng, hand = _fresh(n), _fresh(n)
    before = _policy(16, 16, 3, 'relu', 83)
    eng.set_opponent_network(before, 0x3 << 4)             # a previously set policy network comes back afterwards
    gl, gr = league.play_networks(eng, learner, frozen, T, chunk=4)
    assert eng.network is None and eng.opponent_network is before and eng.opponent_mask == 0x3 << 4
    assert eng.kernel_name().endswith('policy network>')
    hand.set_network(learner, 'left')
    hand.set_opponent_network(frozen, 'right')
    hand.reset()
    hand.rollout(4, with_obs=False); hand.rollout(4, with_obs=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.arena, hand.arena)
    assert torch.equal(gl, hand.score_left.to(torch.int64)) and torch.equal(gr, hand.score_right.to(torch.int64))
    snap = learner.snapshot(deterministic=True)
    gl2, gr2 = league.play_networks(eng, snap, learner, T, chunk=8)       # policy against policy, either side
    assert tuple(gl2.shape) == tuple(gr2.shape) == (n,)
    idx = eng.rollout(1, net_index=True, with_obs=False)['net_index'][0]
    assert (idx[:, 4:6] >= 0).all() and (idx[:, :4] == -1).all() and (idx[:, 6:] == -1).all()
    eng.close(); hand.close()


def test_vec_env_with_a_policy_opponent():
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    n, T = 4, 8
    opp = _policy(32, 16, 6, 'tanh', 91)
    env = Soccer2DMatchVecEnv(n, opponent=opp, obs='agent', noise=True)
    assert env.engine.kernel_name().endswith('policy network>') and env.engine.network is opp
    obs = env.reset()
    assert tuple(obs.shape) == (n, 11, 224)
    twin = _fresh(n)
    twin.set_network(opp, 'right')
    twin.reset()
    torch.manual_seed(0)
    for _ in range(T):
        act = torch.zeros((n, 11, 3), device='cuda:0')
        act[..., 0] = 1.0
        act[..., 1] = torch.rand((n, 11), device='cuda:0') * 100
        obs, rew, done, info = env.step(act)
        full = torch.zeros((n, 22, 3), device='cuda:0')
        full[:, :11] = act
        twin.step(full)
    torch.cuda.synchronize()
    assert tuple(obs.shape) == (n, 11, 224) and tuple(rew.shape) == (n, 11)
    assert torch.equal(env.engine.arena, twin.arena)
    twin.close()


def test_ppo_example_one_iteration():
    sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'examples'))
    try:
        import ppo_match_selfplay as ex
    finally:
        sys.path.pop(0)
    stats = ex.main(['--num-matches', '4', '--steps', '8', '--iterations', '1', '--epochs', '1', '--minibatches', '2',
                     '--eval-every', '1', '--eval-cycles', '8', '--hidden', '16', '--seed', '3'])
    last = stats[-1]
    for key in ('policy_loss', 'value_loss', 'entropy', 'approx_kl'):
        assert np.isfinite(last[key]), (key, last)
    assert 'eval_goals_learner' in last
