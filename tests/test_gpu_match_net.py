"""11v11 network slots on the GPU (s2d_match_set_network / s2d_match_rollout_net): the in-kernel Q-network chooses, for every
network slot, the index the host restatement (tests/match_net_ref.c on tests/agent_obs_ref.c's rows, numpy Philox draws) chooses,
bit for bit, on both rule sets with noise on; the recorded rows are the agent observations of the start-of-cycle state; the
recorded actions drive the CPU oracle to the same states; mirrored states give mirrored slots the same index; random slots and
caller rows are untouched; exploration is uniform; a captured graph acts with the weights, epsilon and table at replay."""
import numpy as np
import pytest

import agent_obs as A
import match_net as MN
import match_oracle as MO
from test_gpu_match import _pair, assert_match_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
ALL = 0x3FFFFF


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('match_net')
    return MN.build(d), A.build(d)


def _module(h1, h2, k, seed, scale=1.0):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(224, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                            torch.nn.Linear(h2, k))
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(scale)
    return m.to('cuda:0')


def _table(k, seed):
    """K rows of (command, a, b): dashes, turns, kicks, tackles and catches with varied arguments"""
    rng = np.random.default_rng(seed)
    cmd = rng.integers(1, 6, k).astype(np.float32)
    a = rng.uniform(-100, 100, k).astype(np.float32)
    b = rng.uniform(-180, 180, k).astype(np.float32)
    return np.stack([cmd, a, b], axis=1)


def _actor(h1, h2, k, eps, seed=1):
    from soccer2d_amd.actor import MatchQNetActor
    return MatchQNetActor.from_module(_module(h1, h2, k, seed), _table(k, seed), epsilon=eps)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, tag):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f'{tag}: {len(bad)} entries differ; first at {i}: gpu={got[i]!r} host={want[i]!r}')


def _orc_state(orc, rows=None):
    s = {k: orc.get(k) for k in A.OBJ_PLANES + A.ENV_WORDS}
    return s if rows is None else {k: v[rows] for k, v in s.items()}


def _eng_state(eng):
    return {k: getattr(eng, k).cpu().numpy() for k in A.OBJ_PLANES + A.ENV_WORDS}


def _slots(mask):
    return [i for i in range(22) if (mask >> i) & 1]


def _closed_loop(refs, n, T, actor, mask, obs_mask, general, monkeypatch, sample=None, ctl=None, launches=1):
    """launches x T cycles; per cycle: recorded rows == host rows of the oracle state, recorded indices == host indices,
    recorded actions == table[index] for network slots, and the oracle driven by the recorded actions ends where the engine does"""
    L, AL = refs
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    eng, orc = _pair(n, noise=True, seed=23 if general else 0x5EED)
    if ctl is not None:
        eng.set_controllers(ctl)
    eng.set_network(actor, mask)
    assert eng.kernel_name().endswith('network>') and ('general' in eng.kernel_name()) == general
    eng.reset(); orc.reset()
    prm = A.params(eng.cfg)
    params = actor.params.cpu().numpy()
    table = actor.table.cpu().numpy()
    slots = _slots(mask)
    rows = np.arange(n) if sample is None else np.arange(sample)
    seen = set()
    for _ in range(launches):
        out = eng.rollout(T, record_actions=True, net_index=True, agent_obs=obs_mask, with_obs=False)
        rec, idx = out['actions'].cpu().numpy(), out['net_index'].cpu().numpy()
        aobs = out['agent_obs'].cpu().numpy() if obs_mask is not None else None
        for t in range(T):
            s = _orc_state(orc, rows)
            host_rows = A.observations(AL, s, prm, mask)
            if aobs is not None:
                _same(aobs[t][rows], A.observations(AL, s, prm, obs_mask), f'agent_obs t={t}')
            want = MN.indices(L, host_rows, params, actor.hidden1, actor.hidden2, actor.n_actions, actor.epsilon,
                              eng.cfg.seed, rows + eng.cfg.env_id_offset, orc.get('tick')[rows], slots)
            _same(idx[t][rows][:, slots], want, f'net_index t={t}')
            assert (idx[t][:, [i for i in range(22) if i not in slots]] == -1).all()
            _same(rec[t][:, slots], table[idx[t][:, slots]], f'actions t={t}')
            seen.update(np.unique(s['mode']).tolist())
            orc.step(rec[t])
    assert_match_same(eng, orc, 'end state')
    eng.close()
    return seen


@pytest.mark.parametrize('general', [False, True])
def test_closed_loop_all_slots_bit_exact(refs, general, monkeypatch):
    """1024 matches x 48 cycles, all 22 slots on one network, epsilon 0.3, every record on"""
    actor = _actor(32, 16, 12, eps=0.3, seed=3)
    _closed_loop(refs, 1024, 24, actor, ALL, ALL, general, monkeypatch, launches=2)


def test_full_size_left_network_right_scripted(refs, monkeypatch):
    """8192 matches x 64 cycles, the left team on the network, the right one scripted, no row record: the oracle replay covers
    every match, the host indices the first 1024"""
    actor = _actor(16, 16, 5, eps=0.1, seed=5)
    _closed_loop(refs, 8192, 64, actor, 0x7FF, None, False, monkeypatch, sample=1024,
                 ctl={'left': 'external', 'right': 'scripted'})


def test_mirrored_states_give_mirrored_slots_the_same_index():
    from soccer2d_amd.match import MatchEngine
    from test_gpu_match_agent_obs import TYPES, _write
    n = 4096
    ids = [0] + list(range(1, 11)) + [0] + list(range(7, 17))
    a = MatchEngine(n, 'cuda:0', player_types=TYPES, player_type_id=ids)
    b = MatchEngine(n, 'cuda:0', player_types=TYPES, player_type_id=ids[11:] + ids[:11])
    s = A.random_state(np.random.default_rng(9), n)
    s['mode'][:] = 2                      # PlayOn: the cycle that follows plays an ordinary ball
    s['mode_side'][:] = 0
    s['ball_holder'][:] = 0
    _write(a, s)
    _write(b, A.mirror(s))
    actor = _actor(64, 64, 16, eps=0.0, seed=7)
    a.set_network(actor); b.set_network(actor)
    ia = a.rollout(1, net_index=True, with_obs=False)['net_index'][0].cpu().numpy()
    ib = b.rollout(1, net_index=True, with_obs=False)['net_index'][0].cpu().numpy()
    assert np.array_equal(ia[:, :11], ib[:, 11:]) and np.array_equal(ia[:, 11:], ib[:, :11])
    assert len(np.unique(ia)) > 4
    a.close(); b.close()


def test_random_slots_and_caller_rows_are_untouched():
    from soccer2d_amd.match import MatchEngine
    n, T = 2048, 16
    actor = _actor(32, 32, 8, eps=0.2, seed=11)
    # random slots draw what they draw without a network
    a = MatchEngine(n, 'cuda:0', noise=True)
    b = MatchEngine(n, 'cuda:0', noise=True)
    for e in (a, b):
        e.set_controllers({'left': 'random', 'right': 'random'})
        e.reset()
    b.set_network(actor, 'left')
    ra = a.rollout(T, record_actions=True, with_obs=False)['actions'].cpu().numpy()
    rb = b.rollout(T, record_actions=True, with_obs=False)['actions'].cpu().numpy()
    _same(rb[:, :, 11:], ra[:, :, 11:], 'random slots')
    assert not np.array_equal(_bits(rb[:, :, :11]), _bits(ra[:, :, :11]))
    # caller rows of network slots are never read
    outs = []
    for fill in (0.0, float('nan')):
        e = MatchEngine(n, 'cuda:0', noise=True)
        e.set_controllers({'left': 'external', 'right': 'scripted'})
        e.set_network(actor, 'left')
        e.reset()
        acts = torch.full((T, n, 22, 3), fill, device='cuda:0')
        o = e.rollout(T, actions=acts, record_actions=True, net_index=True)
        outs.append((o['actions'].cpu().numpy(), o['net_index'].cpu().numpy(), e.arena.cpu().numpy()))
        e.close()
    for x, y in zip(*outs):
        _same(x, y, 'NaN caller rows')
    # without a network the engine runs its old kernels again
    b.set_network(None)
    assert not b.kernel_name().endswith('network>')
    # records without a network: every index -1, the rows of the start-of-cycle state
    start = b.agent_observations('left').clone()
    o = b.rollout(2, net_index=True, agent_obs='left', with_obs=False)
    assert (o['net_index'] == -1).all() and torch.equal(o['agent_obs'][0], start)
    a.close(); b.close()


def test_exploration_uniform_greedy_and_counter_wrap(refs):
    from soccer2d_amd.match import MatchEngine
    L, AL = refs
    n, T, k = 4096, 8, 5
    eng = MatchEngine(n, 'cuda:0', noise=True)
    actor = _actor(16, 32, k, eps=1.0, seed=13)
    eng.set_network(actor)
    eng.reset()
    idx = eng.rollout(T, net_index=True, with_obs=False)['net_index'].cpu().numpy()
    counts = np.bincount(idx.reshape(-1), minlength=k)
    expect = idx.size / k
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert chi2 < 20.5, (counts, chi2)                     # 4 degrees of freedom, p ~ 4e-4
    # epsilon 0: the greedy index of the recorded row, always
    actor.epsilon = 0.0
    out = eng.rollout(T, net_index=True, agent_obs='all', with_obs=False)
    rows, idx = out['agent_obs'].cpu().numpy(), out['net_index'].cpu().numpy()
    g = MN.argmax(L, MN.forward(L, rows[:, :512], actor.params.cpu().numpy(), 16, 32, k))
    assert np.array_equal(idx[:, :512], g)
    # the tick counter past 2^31 (the int32 view turns negative) and 2^32 (it wraps): the draws follow it
    actor.epsilon = 0.5
    start = np.array([2 ** 31 - 3, -3, 7], dtype=np.int32)[np.arange(n) % 3]
    eng.tick.copy_(torch.from_numpy(start))
    out = eng.rollout(T, net_index=True, agent_obs='all', with_obs=False)
    rows, idx = out['agent_obs'].cpu().numpy(), out['net_index'].cpu().numpy()
    params = actor.params.cpu().numpy()
    for t in range(T):
        tick = (start.astype(np.int64) + t) & 0xFFFFFFFF
        want = MN.indices(L, rows[t], params, 16, 32, k, 0.5, eng.cfg.seed, np.arange(n), tick, range(22))
        _same(idx[t], want, f'wrap t={t}')
    eng.close()


def test_graph_replay_acts_with_new_weights_epsilon_and_table(refs):
    from soccer2d_amd.match import MatchEngine
    n, T = 1024, 4
    actor = _actor(32, 32, 6, eps=0.3, seed=17)
    module = actor._module
    a = MatchEngine(n, 'cuda:0', noise=True)
    b = MatchEngine(n, 'cuda:0', noise=True)
    for e in (a, b):
        e.set_network(actor)
        e.reset()
    out = a.alloc_rollout(T, with_obs=False, record_actions=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.rollout(T, out=out, record_actions=True, net_index=True, with_obs=False)
    torch.cuda.current_stream().wait_stream(s)
    b.rollout(T, record_actions=True, with_obs=False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.rollout(T, out=out, record_actions=True, net_index=True, with_obs=False)
    first = out['net_index'].clone()
    with torch.no_grad():
        for p in module.parameters():
            p.add_(torch.randn_like(p) * 0.5)
    actor.sync()
    actor.epsilon = 0.0
    actor.set_table(_table(6, 99))
    g.replay()
    ob = b.rollout(T, record_actions=True, net_index=True, with_obs=False)
    torch.cuda.synchronize()
    assert torch.equal(out['net_index'], ob['net_index']) and torch.equal(out['actions'], ob['actions'])
    assert torch.equal(a.arena, b.arena)
    assert not torch.equal(first, out['net_index'])
    tab = actor.table.cpu().numpy()
    idx = out['net_index'].cpu().numpy()
    _same(out['actions'].cpu().numpy(), tab[idx], 'new table')
    a.close(); b.close()


@pytest.mark.parametrize('h1', [16, 32, 48, 64])
@pytest.mark.parametrize('h2', [16, 32, 48, 64])
def test_shapes_and_sizes(refs, h1, h2):
    from soccer2d_amd.match import MatchEngine
    L, AL = refs
    for j, k in enumerate((1, 5, 16, 64)):
        n = (1, 7, 1001)[(h1 // 16 + h2 // 16 + j) % 3]
        eng = MatchEngine(n, 'cuda:0', noise=True, seed=h1 + h2 + k)
        actor = _actor(h1, h2, k, eps=0.25, seed=h1 * 100 + h2 + k)
        mask = (0x2A5A5, ALL, 0x7FF)[j % 3]
        eng.set_network(actor, mask)
        eng.reset()
        eng.rollout(3, with_obs=False)
        s = _eng_state(eng)
        tick = eng.tick.cpu().numpy()
        out = eng.rollout(1, net_index=True, agent_obs=mask, record_actions=True, with_obs=False)
        rows = out['agent_obs'][0].cpu().numpy()
        _same(rows, A.observations(AL, s, A.params(eng.cfg), mask), f'rows {h1}-{h2}-{k} n={n}')
        want = MN.indices(L, rows, actor.params.cpu().numpy(), h1, h2, k, 0.25, eng.cfg.seed, np.arange(n), tick, _slots(mask))
        _same(out['net_index'][0].cpu().numpy()[:, _slots(mask)], want, f'index {h1}-{h2}-{k} n={n}')
        eng.close()


def test_rejections_leave_the_engine_unchanged():
    import ctypes as C
    from soccer2d_amd import _capi_match as M
    from soccer2d_amd.match import MatchEngine
    n = 64
    eng = MatchEngine(n, 'cuda:0', noise=True)
    actor = _actor(32, 32, 8, eps=0.1, seed=21)
    eng.set_network(actor, 'left')
    eng.reset()
    before = eng.arena.clone()
    good = actor.c_struct(0x7FF)
    bad = []
    for field, value in (('h1', 24), ('h2', 80), ('n_actions', 0), ('n_actions', 65), ('slot_mask', 0), ('slot_mask', 1 << 22),
                         ('params', actor.params.data_ptr() + 4), ('params', None), ('epsilon', None),
                         ('table', actor.table.data_ptr() + 2), ('table', None)):
        s = M.S2DMatchNet.from_buffer_copy(good)
        setattr(s, field, value)
        bad.append(s)
    for s in bad:
        assert eng.lib.s2d_match_set_network(eng._h, C.byref(s)) != 0
    assert eng.kernel_name().endswith('network>')
    torch.cuda.synchronize()
    assert torch.equal(before, eng.arena)
    # the network is still the one set before the rejected calls: left slots on it, right slots random
    idx = eng.rollout(1, net_index=True, with_obs=False)['net_index'][0].cpu().numpy()
    assert (idx[:, :11] >= 0).all() and (idx[:, 11:] == -1).all()
    buf = torch.empty((1, n, 11, 224), device='cuda:0')
    st = eng._stream()
    ro = M.S2DMatchRollout()
    assert eng.lib.s2d_match_rollout_net(eng._h, 1, None, C.byref(ro), None, None, 0, C.c_void_p(buf.data_ptr()), st) != 0
    assert eng.lib.s2d_match_rollout_net(eng._h, 1, None, C.byref(ro), None, None, 1 << 22, C.c_void_p(buf.data_ptr()), st) != 0
    assert eng.lib.s2d_match_rollout_net(eng._h, 1, None, C.byref(ro), None, None, 0x7FF, C.c_void_p(buf.data_ptr() + 4), st) != 0
    with pytest.raises(ValueError):
        eng.set_network(actor, 0)
    with pytest.raises(ValueError):
        eng.set_network(actor, 1 << 22)
    eng.set_network(None)
    assert not eng.kernel_name().endswith('network>')
    eng.close()


def test_vec_env_network_opponent():
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    n = 256
    actor = _actor(32, 32, 8, eps=0.0, seed=31)
    env = Soccer2DMatchVecEnv(n, opponent=actor, obs='agent', noise=True)
    assert env.observation_space.shape == (11, 224) and env.action_space.shape == (11, 3)
    obs = env.reset()
    assert obs.shape == (n, 11, 224)
    assert env.engine.kernel_name().endswith('network>') and env.engine.network_mask == 0x3FF800
    for _ in range(5):
        obs, rew, done, info = env.step(torch.zeros((n, 11, 3), device='cuda:0'))
        assert obs.shape == (n, 11, 224) and rew.shape == (n, 11)
        assert torch.equal(obs, env.engine.agent_observations('left'))
    env.close()
