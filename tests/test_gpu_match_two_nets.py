"""11v11 with two in-kernel networks (s2d_match_set_network + s2d_match_set_opponent_network): every slot chooses, bit for bit
and with noise on, the index the host restatement (tests/match_net_ref.c on tests/agent_obs_ref.c's rows, numpy Philox draws)
chooses with the parameters, K, epsilon and table of the network the slot belongs to -- in closed loop against the CPU oracle, on
masks whose tiles would straddle the two networks, at the widest shapes, under graph replay; the two setters are symmetric and
independent, reject what they must and leave the engine unchanged; league.play_networks plays learner versus frozen snapshot."""
import numpy as np
import pytest

import agent_obs as A
import match_net as MN
from test_gpu_match import _pair, assert_match_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
ALL, LEFT, RIGHT = 0x3FFFFF, 0x7FF, 0x3FF800
EVEN, ODD = 0x155555, 0x2AAAAA


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('match_two_nets')
    return MN.build(d), A.build(d)


def _module(h1, h2, k, seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(224, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                            torch.nn.Linear(h2, k))
    return m.to('cuda:0')


def _table(k, seed):
    rng = np.random.default_rng(seed)
    cmd = rng.integers(1, 6, k).astype(np.float32)
    a = rng.uniform(-100, 100, k).astype(np.float32)
    b = rng.uniform(-180, 180, k).astype(np.float32)
    return np.stack([cmd, a, b], axis=1)


def _actor(h1, h2, k, eps, seed):
    from soccer2d_amd.actor import MatchQNetActor
    return MatchQNetActor.from_module(_module(h1, h2, k, seed), _table(k, 1000 + seed), epsilon=eps)


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


def _orc_state(orc):
    return {k: orc.get(k) for k in A.OBJ_PLANES + A.ENV_WORDS}


def _host(actor):
    """what the host restatement needs of an actor, as it is now"""
    return dict(params=actor.params.cpu().numpy(), table=actor.table.cpu().numpy(), h1=actor.hidden1, h2=actor.hidden2,
                k=actor.n_actions, eps=actor.epsilon)


def _want(L, rows, net, seed, gid, tick, slots):
    return MN.indices(L, rows, net['params'], net['h1'], net['h2'], net['k'], net['eps'], seed, gid, tick, slots)


def _install(eng, a, mask_a, b, mask_b, swap=False):
    """a as the network and b as the opponent network; swap: the other way round"""
    if swap:
        eng.set_network(b, mask_b)
        eng.set_opponent_network(a, mask_a)
    else:
        eng.set_network(a, mask_a)
        eng.set_opponent_network(b, mask_b)


def _closed_loop_two(refs, n, T, a, mask_a, b, mask_b, obs_mask, general, monkeypatch, launches=1, swap=False):
    """launches x T cycles with two networks; per cycle: recorded rows == host rows of the oracle state; the recorded index of
    every slot == the host index under its own network's parameters, K and epsilon; recorded actions == its own table's row; and
    the oracle driven by the recorded actions ends where the engine does"""
    L, AL = refs
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    eng, orc = _pair(n, noise=True, seed=23 if general else 0x5EED)
    _install(eng, a, mask_a, b, mask_b, swap)
    name = eng.kernel_name()
    assert name.endswith('two networks>') and ('general' in name) == general, name
    eng.reset(); orc.reset()
    prm = A.params(eng.cfg)
    nets = [(_host(a), mask_a, _slots(mask_a), 'A'), (_host(b), mask_b, _slots(mask_b), 'B')]
    others = [i for i in range(22) if not ((mask_a | mask_b) >> i) & 1]
    gid = np.arange(n) + eng.cfg.env_id_offset
    for launch in range(launches):
        out = eng.rollout(T, record_actions=True, net_index=True, agent_obs=obs_mask, with_obs=False)
        rec, idx, aobs = out['actions'].cpu().numpy(), out['net_index'].cpu().numpy(), out['agent_obs'].cpu().numpy()
        for t in range(T):
            s = _orc_state(orc)
            tag = f'launch {launch} t={t}'
            _same(aobs[t], A.observations(AL, s, prm, obs_mask), f'agent_obs {tag}')
            for net, mask, slots, who in nets:
                want = _want(L, A.observations(AL, s, prm, mask), net, eng.cfg.seed, gid, orc.get('tick'), slots)
                _same(idx[t][:, slots], want, f'net_index of {who} {tag}')
                _same(rec[t][:, slots], net['table'][idx[t][:, slots]], f'actions of {who} {tag}')
            assert (idx[t][:, others] == -1).all()
            orc.step(rec[t])
    assert_match_same(eng, orc, 'end state')
    eng.close()


@pytest.mark.parametrize('general', [False, True])
def test_closed_loop_two_networks_bit_exact(refs, general, monkeypatch):
    """130 matches (65 waves) x 8 cycles x 2 launches: A = 16-48-5 on the left at epsilon 0.3, B = 64-16-64 on the right at 0.1"""
    a = _actor(16, 48, 5, eps=0.3, seed=3)
    b = _actor(64, 16, 64, eps=0.1, seed=4)
    _closed_loop_two(refs, 130, 8, a, LEFT, b, RIGHT, ALL, general, monkeypatch, launches=2)


STRADDLE = {
    'interleaved':        dict(n=64, a=(32, 32, 7), mask_a=EVEN, b=(48, 16, 9), mask_b=ODD, obs=ALL),          # 11 rows each: 8 + 3
    'one and twenty-one': dict(n=64, a=(32, 32, 7), mask_a=0x1, b=(48, 16, 9), mask_b=ALL & ~0x1, obs=ALL),      # B: 8 + 8 + 5
    'recorded only':      dict(n=64, a=(32, 32, 7), mask_a=LEFT, b=(48, 16, 9), mask_b=(1 << 11) | (1 << 21),
                               obs=(1 << 5) | (1 << 12) | (1 << 13)),                                         # rows of A, rows of neither
    'K 1 and K 64':       dict(n=64, a=(16, 32, 1), mask_a=LEFT, b=(32, 64, 64), mask_b=RIGHT, obs=ALL),
    'K 64 and K 1':       dict(n=64, a=(32, 64, 64), mask_a=EVEN, b=(16, 32, 1), mask_b=ODD, obs=ALL),
    'odd match count':    dict(n=129, a=(32, 32, 7), mask_a=EVEN, b=(48, 16, 9), mask_b=ODD, obs=ALL),            # last wave: one match
}


@pytest.mark.parametrize('case', sorted(STRADDLE))
def test_tiles_that_would_straddle_two_networks(refs, case, monkeypatch):
    """64 matches x 4 cycles on masks where a 16-row tile filled in slot order would hold rows of both networks"""
    c = STRADDLE[case]
    a = _actor(*c['a'], eps=0.3, seed=11)
    b = _actor(*c['b'], eps=0.15, seed=12)
    _closed_loop_two(refs, c['n'], 4, a, c['mask_a'], b, c['mask_b'], c['obs'], False, monkeypatch,
                     swap=case in ('one and twenty-one', 'K 64 and K 1'))


def _fresh(n, **kw):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(n, 'cuda:0', noise=True, **kw)
    return eng


def _run(eng, T, actions=None, agent_obs='all'):
    eng.reset()
    out = eng.rollout(T, actions=actions, record_actions=True, net_index=True, agent_obs=agent_obs, with_obs=False)
    torch.cuda.synchronize()
    return out


def test_symmetry_and_independence():
    n, T = 256, 8
    a = _actor(32, 48, 6, eps=0.3, seed=21)
    b = _actor(48, 32, 11, eps=0.1, seed=22)
    # the two setters are symmetric: which of them holds which network changes no bit
    x, x2 = _fresh(n), _fresh(n)
    _install(x, a, LEFT, b, RIGHT)
    _install(x2, a, LEFT, b, RIGHT, swap=True)
    assert x.kernel_name() == x2.kernel_name() and x.kernel_name().endswith('two networks>')
    ox, ox2 = _run(x, T), _run(x2, T)
    for k in ('actions', 'net_index', 'agent_obs', 'reward', 'mode', 'done'):
        assert torch.equal(ox[k], ox2[k]), k
    assert torch.equal(x.arena, x2.arena)
    assert (ox['net_index'] >= 0).all() and int(ox['net_index'][..., 11:].max()) > 5
    # a slot's index is a function of its own network only: A against the same right-team actions from outside
    y = _fresh(n)
    y.set_controllers({'left': 'external', 'right': 'external'})
    y.set_network(a, 'left')
    assert y.kernel_name().endswith('network>') and not y.kernel_name().endswith('two networks>')
    oy = _run(y, T, actions=ox['actions'])
    assert torch.equal(oy['net_index'][..., :11], ox['net_index'][..., :11]) and (oy['net_index'][..., 11:] == -1).all()
    assert torch.equal(oy['actions'], ox['actions']) and torch.equal(y.arena, x.arena)
    # the opponent alone is the network alone
    p, q = _fresh(n), _fresh(n)
    p.set_opponent_network(b, ODD)
    q.set_network(b, ODD)
    assert p.kernel_name() == q.kernel_name() and p.kernel_name().endswith('network>')
    op, oq = _run(p, T, agent_obs='left'), _run(q, T, agent_obs='left')
    for k in ('actions', 'net_index', 'agent_obs'):
        assert torch.equal(op[k], oq[k]), k
    assert torch.equal(p.arena, q.arena)
    assert (op['net_index'][..., 1::2] >= 0).all() and (op['net_index'][..., 0::2] == -1).all()
    for e in (x, x2, y, p, q):
        e.close()


@pytest.mark.parametrize('general', [False, True])
def test_widest_shapes_both_networks(refs, general, monkeypatch):
    """both networks 64-64-64 on 64 matches x 2 cycles: the largest LDS request (the general kernels leave less room)"""
    a = _actor(64, 64, 64, eps=0.2, seed=31)
    b = _actor(64, 64, 64, eps=0.2, seed=32)
    _closed_loop_two(refs, 64, 2, a, LEFT, b, RIGHT, ALL, general, monkeypatch)


def test_graph_replay_follows_the_opponents_new_weights_epsilon_and_table(refs):
    L, AL = refs
    n, T = 256, 4
    a = _actor(32, 32, 6, eps=0.3, seed=41)
    b = _actor(48, 16, 9, eps=0.2, seed=42)
    eng = _fresh(n)
    _install(eng, a, LEFT, b, RIGHT)
    eng.reset()
    out = eng.alloc_rollout(T, with_obs=False, record_actions=True)
    kw = dict(out=out, record_actions=True, net_index=True, agent_obs='all', with_obs=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.rollout(T, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.rollout(T, **kw)
    gid = np.arange(n) + eng.cfg.env_id_offset

    def check(tick0, tag):
        rows, idx, rec = (out[k].cpu().numpy() for k in ('agent_obs', 'net_index', 'actions'))
        for actor, slots in ((a, _slots(LEFT)), (b, _slots(RIGHT))):
            net = _host(actor)
            for t in range(T):
                want = _want(L, rows[t][:, slots], net, eng.cfg.seed, gid, tick0 + t, slots)
                _same(idx[t][:, slots], want, f'{tag} t={t} slots {slots[0]}..')
                _same(rec[t][:, slots], net['table'][idx[t][:, slots]], f'{tag} actions t={t} slots {slots[0]}..')
        return idx

    eng.reset()
    tick0 = eng.tick.cpu().numpy().astype(np.int64)
    g.replay()
    torch.cuda.synchronize()
    check(tick0, 'first replay')
    a_before, b_before = _host(a), _host(b)
    with torch.no_grad():
        for p in b._module.parameters():
            p.add_(torch.randn_like(p) * 0.5)
    b.sync()
    b.epsilon = 0.6
    b.set_table(_table(9, 99))
    eng.reset()
    tick0 = eng.tick.cpu().numpy().astype(np.int64)
    g.replay()
    torch.cuda.synchronize()
    idx = check(tick0, 'second replay')                    # B by the new values, A by the ones it always had
    assert np.array_equal(a_before['params'], _host(a)['params']) and a.epsilon == 0.3
    # B's old values would have chosen otherwise: the replay did read the new ones
    right = _slots(RIGHT)
    old = _want(L, out['agent_obs'][0].cpu().numpy()[:, right], b_before, eng.cfg.seed, gid, tick0, right)
    assert not np.array_equal(idx[0][:, right], old)
    assert not np.array_equal(b_before['table'], _host(b)['table'])
    eng.close()


def test_rejections_leave_the_engine_unchanged():
    import ctypes as C
    from soccer2d_amd import _capi_match as M
    from soccer2d_amd.actor import MatchQNetActor
    n = 64
    eng = _fresh(n)
    a = _actor(32, 32, 8, eps=0.1, seed=51)
    b = _actor(16, 48, 5, eps=0.1, seed=52)
    _install(eng, a, LEFT, b, RIGHT)
    eng.reset()
    before = eng.arena.clone()
    lib, h = eng.lib, eng._h
    good = b.c_struct(RIGHT)
    bad = []
    for field, value in (('h1', 24), ('h2', 80), ('n_actions', 0), ('n_actions', 65), ('slot_mask', 0), ('slot_mask', 1 << 22),
                         ('params', b.params.data_ptr() + 4), ('params', None), ('epsilon', None),
                         ('table', b.table.data_ptr() + 2), ('table', None),
                         ('slot_mask', RIGHT | 1), ('slot_mask', 1 << 10), ('slot_mask', ALL)):     # overlaps the network's mask
        s = M.S2DMatchNet.from_buffer_copy(good)
        setattr(s, field, value)
        bad.append(s)
    for s in bad:
        assert lib.s2d_match_set_opponent_network(h, C.byref(s)) == -1
        assert lib.s2d_last_error()
    # the other order: the network's mask against the set opponent's
    for mask in (LEFT | (1 << 11), 1 << 21, ALL):
        assert lib.s2d_match_set_network(h, C.byref(a.c_struct(mask))) == -1
    with pytest.raises(ValueError):
        eng.set_opponent_network(b, 'all')
    with pytest.raises(ValueError):
        eng.set_network(a, 'all')
    with pytest.raises(ValueError):
        eng.set_opponent_network(MatchQNetActor(16, 16, 4, obs='see'), 'right')
    assert eng.kernel_name().endswith('two networks>')
    torch.cuda.synchronize()
    assert torch.equal(before, eng.arena)
    assert eng.network is a and eng.opponent_network is b and (eng.network_mask, eng.opponent_mask) == (LEFT, RIGHT)
    # the pair set before the rejected calls still acts, each on its own table
    out = eng.rollout(1, net_index=True, record_actions=True, with_obs=False)
    idx, rec = out['net_index'][0].cpu().numpy(), out['actions'][0].cpu().numpy()
    assert (idx[:, :11] >= 0).all() and (idx[:, :11] < 8).all() and (idx[:, 11:] >= 0).all() and (idx[:, 11:] < 5).all()
    _same(rec[:, :11], a.table.cpu().numpy()[idx[:, :11]], 'the network acts')
    _same(rec[:, 11:], b.table.cpu().numpy()[idx[:, 11:]], 'the opponent acts')
    # s2d_match_set_network(h, NULL) clears the network only
    assert lib.s2d_match_set_network(h, None) == 0
    assert eng.kernel_name().endswith('network>') and not eng.kernel_name().endswith('two networks>')
    idx = eng.rollout(1, net_index=True, with_obs=False)['net_index'][0].cpu().numpy()
    assert (idx[:, 11:] >= 0).all() and (idx[:, :11] == -1).all()
    # ... and s2d_match_set_opponent_network(h, NULL) the opponent only
    eng.set_network(a, 'left')
    eng.set_opponent_network(None)
    assert eng.kernel_name().endswith('network>') and not eng.kernel_name().endswith('two networks>')
    idx = eng.rollout(1, net_index=True, with_obs=False)['net_index'][0].cpu().numpy()
    assert (idx[:, :11] >= 0).all() and (idx[:, 11:] == -1).all()
    # a see network is the engine's only one: it clears both, and no opponent can be set beside it
    eng.set_opponent_network(b, 'right')
    assert eng.kernel_name().endswith('two networks>')
    eng.enable_vision()
    see = MatchQNetActor(16, 16, 3, epsilon=0.0, obs='see')
    eng.set_network(see, 'left')
    assert eng.kernel_name().endswith('see network>') and eng.opponent_network is None and eng.opponent_mask == 0
    assert lib.s2d_match_set_opponent_network(h, C.byref(good)) == -1 and b'see network' in lib.s2d_last_error()
    with pytest.raises(ValueError):
        eng.set_opponent_network(b, 'right')
    assert eng.kernel_name().endswith('see network>')
    idx = eng.rollout(1, net_index=True, with_obs=False)['net_index'][0].cpu().numpy()
    assert (idx[:, :11] >= 0).all() and (idx[:, 11:] == -1).all()          # the opponent is gone
    eng.set_network(None)
    assert not eng.kernel_name().endswith('network>')
    eng.close()


def test_league_play_networks(refs):
    from soccer2d_amd import league
    L, AL = refs
    n, T, chunk = 128, 40, 16
    a = _actor(32, 32, 8, eps=0.2, seed=61)
    frozen = a.snapshot()
    assert frozen.epsilon == 0.0 and torch.equal(frozen.params, a.params) and frozen.params.data_ptr() != a.params.data_ptr()
    eng, hand = _fresh(n), _fresh(n)
    gl, gr = league.play_networks(eng, a, frozen, T, chunk=chunk)
    assert gl.dtype == gr.dtype == torch.int64 and tuple(gl.shape) == tuple(gr.shape) == (n,)
    assert torch.equal(gl, eng.score_left.to(torch.int64)) and torch.equal(gr, eng.score_right.to(torch.int64))   # reset: 0 : 0
    assert eng.network is None and eng.opponent_network is None and not eng.kernel_name().endswith('network>')
    # the same match-up by hand
    hand.set_network(a, 'left')
    hand.set_opponent_network(frozen, 'right')
    hand.reset()
    for t in (16, 16, 8):
        hand.rollout(t, with_obs=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.arena, hand.arena)
    assert torch.equal(gl, hand.score_left.to(torch.int64)) and torch.equal(gr, hand.score_right.to(torch.int64))
    assert int(eng.stats[0]) == n * T
    # a previously set network is restored
    other = _actor(16, 16, 4, eps=0.0, seed=62)
    eng.set_network(other, EVEN)
    gl2, gr2 = league.play_networks(eng, a, frozen, T, chunk=chunk)
    assert torch.equal(gl2, gl) and torch.equal(gr2, gr)
    assert eng.network is other and eng.network_mask == EVEN and eng.opponent_network is None
    idx = eng.rollout(1, net_index=True, with_obs=False)['net_index'][0]
    assert (idx[:, 0::2] >= 0).all() and (idx[:, 1::2] == -1).all()
    table = league.League(2)
    table.update(torch.zeros(n, dtype=torch.int64), torch.ones(n, dtype=torch.int64), gl.cpu(), gr.cpu())
    assert int(table.games.sum()) == 2 * n
    # the learner moves on, the snapshot does not: its slots keep choosing by the old weights
    old = _host(frozen)
    with torch.no_grad():
        for p in a._module.parameters():
            p.add_(torch.randn_like(p) * 0.5)
    a.sync()
    assert not torch.equal(frozen.params, a.params) and np.array_equal(frozen.params.cpu().numpy(), old['params'])
    tick = hand.tick.cpu().numpy()
    out = hand.rollout(1, net_index=True, agent_obs='all', with_obs=False)
    rows, idx = out['agent_obs'][0].cpu().numpy(), out['net_index'][0].cpu().numpy()
    gid = np.arange(n) + hand.cfg.env_id_offset
    right, left = _slots(RIGHT), _slots(LEFT)
    _same(idx[:, right], _want(L, rows[:, right], old, hand.cfg.seed, gid, tick, right), 'the snapshot: old weights')
    _same(idx[:, left], _want(L, rows[:, left], _host(a), hand.cfg.seed, gid, tick, left), 'the learner: new weights')
    eng.close(); hand.close()
