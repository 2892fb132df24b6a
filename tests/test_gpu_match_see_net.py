"""The 11v11 see network on the GPU (s2d_match_set_see_network / s2d_match_rollout_see): the Q-network on see rows inside the cycle
kernel, the vision state stepped there.  Every comparison is bitwise.  The recorded see rows are tests/see_ref.c's on the CPU match
oracle's state and a host vision state; the indices are tests/see_net_ref.c's with tests/match_net.py's draws; the recorded actions
drive the oracle to the engine's end state; one fused launch equals the unfused loop see -> choice -> rollout(1) -> vision_step on a
twin engine; matches that end reset their vision state, sent-off players keep theirs; caller rows of network slots are never read; a
record-only launch leaves the engine as a plain rollout does; every shape; exploration and the tick's wrap; a captured graph acts
with the weights, epsilon and table at replay; rejections leave the engine unchanged; Soccer2DMatchVecEnv with a see opponent."""
import numpy as np
import pytest

import match_net as MN
import match_oracle as MO
import match_see as S
import see_net as SN
from test_gpu_match import _pair, assert_match_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
ALL = 0x3FFFFF
LEFT = 0x7FF


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('see_net')
    return SN.build(d), MN.build(d), S.build(d)


def _module(h1, h2, k, seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(192, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                            torch.nn.Linear(h2, k))
    with torch.no_grad():                                 # stamina (8000) and its capacity (130600) would drown the other words
        m[0].weight[:, [10, 13]] *= 1.0e-4
    return m.to('cuda:0')


def _table(k, seed):
    """K rows of (command, a, b, TurnNeck moment, ChangeView code): dashes, turns, kicks, tackles and catches with varied
    arguments, non-zero neck moments, the four view codes in turn (0 keep, 1 narrow, 2 normal, 3 wide)"""
    rng = np.random.default_rng(seed)
    cmd = rng.integers(1, 6, k).astype(np.float32)
    a = rng.uniform(-100, 100, k).astype(np.float32)
    b = rng.uniform(-180, 180, k).astype(np.float32)
    m = (rng.uniform(5, 70, k) * rng.choice([-1.0, 1.0], k)).astype(np.float32)
    c = ((np.arange(k) + seed) % 4).astype(np.float32)
    return np.stack([cmd, a, b, m, c], axis=1)


def _actor(h1, h2, k, eps, seed=1):
    from soccer2d_amd.actor import MatchQNetActor
    return MatchQNetActor.from_module(_module(h1, h2, k, seed), _table(k, seed), epsilon=eps, obs='see')


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
    return {k: orc.get(k) for k in S.ENGINE_KEYS}


def _planes(eng):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).cpu().numpy() for k in S.VISION_PLANES}


def _prm(eng):
    return S.params(seed=eng.cfg.seed, env_id_offset=eng.cfg.env_id_offset)


def _same_engine(a, b, tag):
    torch.cuda.synchronize()
    assert torch.equal(a.arena, b.arena), f'{tag}: engine state'
    for k in S.VISION_PLANES:
        assert torch.equal(getattr(a, k), getattr(b, k)), f'{tag}: vision plane {k}'


def _closed_loop(refs, eng, orc, actor, mask, obs_mask, T, launches, each_cycle=None):
    """launches x T cycles; per cycle: recorded see rows == the host rows on the oracle state and the host vision state, recorded
    indices == host indices, recorded actions == table[index][:3] for network slots; the oracle is stepped with the record, the
    host vision state with table[index][3:5].  At the end the oracle is where the engine is, and so are the three planes."""
    L, ML, SL = refs
    n = eng.num_envs
    prm = _prm(eng)
    params, table = actor.params.cpu().numpy(), actor.table.cpu().numpy()
    slots, oslots = _slots(mask), _slots(obs_mask)
    others = [i for i in range(22) if i not in slots]
    planes = _planes(eng)
    gid = np.arange(n) + eng.cfg.env_id_offset
    cycle = 0
    for _ in range(launches):
        out = eng.rollout(T, record_actions=True, net_index=True, see_obs=obs_mask, with_obs=False)
        rec, idx, see = out['actions'].cpu().numpy(), out['net_index'].cpu().numpy(), out['see'].cpu().numpy()
        for t in range(T):
            s = dict(_orc_state(orc), **planes)
            rows = S.see(SL, s, prm)
            _same(see[t], rows[:, oslots], f'see rows cycle {cycle}')
            want = SN.indices(L, ML, rows[:, slots], params, actor.hidden1, actor.hidden2, actor.n_actions, actor.epsilon,
                              eng.cfg.seed, gid, s['tick'], slots)
            _same(idx[t][:, slots], want, f'net_index cycle {cycle}')
            assert (idx[t][:, others] == -1).all()
            _same(rec[t][:, slots], table[want][..., :3], f'actions cycle {cycle}')
            orc.step(rec[t])
            va = np.zeros((n, 22, 2), dtype=np.float32)    # the other slots: moment 0, code keep
            va[:, slots] = table[want][..., 3:5]
            done = orc.get('done')
            before = planes
            planes = S.vision_step(SL, dict(_orc_state(orc), **planes), prm, va, done)
            if each_cycle is not None:
                each_cycle(cycle, s, see[t], before, planes, done)
            cycle += 1
    assert_match_same(eng, orc, 'end state')
    got = _planes(eng)
    for k in S.VISION_PLANES:
        _same(got[k], planes[k], f'vision plane {k}')
    return planes


@pytest.mark.parametrize('general', [False, True])
def test_closed_loop_against_the_cpu(refs, general, monkeypatch):
    """64 matches, 2 launches x 12 cycles, all 22 slots on one 192-32-16-12 network, epsilon 0.3, noise on"""
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    eng, orc = _pair(64, noise=True, seed=23 if general else 0x5EED)
    eng.enable_vision()
    actor = _actor(32, 16, 12, eps=0.3, seed=3)
    tab = actor.table.cpu().numpy()
    assert len(np.unique(tab[:, 0])) > 2 and (tab[:, 3] != 0).all() and set(tab[:, 4].tolist()) == {0.0, 1.0, 2.0, 3.0}
    eng.set_network(actor, ALL)
    assert eng.kernel_name().endswith('see network>') and ('general' in eng.kernel_name()) == general
    eng.reset(); orc.reset()
    planes = _closed_loop(refs, eng, orc, actor, ALL, ALL, 12, 2)
    assert (planes['neck'][:, :22] != 0).any() and len(np.unique(planes['view_width'][:, :22])) == 3
    eng.close()


def _unfused_cycle(refs, eng, actor, slots, acts, view):
    """see -> host choice -> rollout(1) -> vision_step(done) on `eng`; acts [N, 22, 3] and view [N, 22, 2] hold the other slots'
    rows (numpy, not modified).  Returns (all 22 see rows, the indices of `slots`)."""
    L, ML, SL = refs
    n = eng.num_envs
    rows = eng.see('all').cpu().numpy()
    tick = eng.tick.cpu().numpy()
    idx = SN.indices(L, ML, rows[:, slots], actor.params.cpu().numpy(), actor.hidden1, actor.hidden2, actor.n_actions,
                     actor.epsilon, eng.cfg.seed, np.arange(n) + eng.cfg.env_id_offset, tick, slots)
    table = actor.table.cpu().numpy()
    a, v = acts.copy(), view.copy()
    a[:, slots] = table[idx][..., :3]
    v[:, slots] = table[idx][..., 3:5]
    eng.rollout(1, actions=torch.from_numpy(a[None]).cuda(), with_obs=False)
    eng.vision_step(torch.from_numpy(v).cuda(), done=True)
    return rows, idx


@pytest.mark.parametrize('n', [9, 3])
def test_fused_equals_unfused(refs, n):
    """the left team on the network, the right one scripted, epsilon 0: one 16-cycle launch against 16 unfused rounds on a twin
    (n = 9: a second workgroup whose only wave is half empty; n = 3: one workgroup, a half-empty second wave)"""
    from soccer2d_amd.match import MatchEngine
    T = 16
    actor = _actor(48, 32, 9, eps=0.0, seed=5)
    a = MatchEngine(n, 'cuda:0', noise=True, seed=77)
    b = MatchEngine(n, 'cuda:0', noise=True, seed=77)
    for e in (a, b):
        e.set_controllers({'left': 'external', 'right': 'scripted'})
        e.enable_vision()
        e.reset()
    a.set_network(actor, 'left')
    out = a.rollout(T, net_index=True, see_obs='all', with_obs=False)
    see, idx = out['see'].cpu().numpy(), out['net_index'].cpu().numpy()
    zeros3, zeros2 = np.zeros((n, 22, 3), dtype=np.float32), np.zeros((n, 22, 2), dtype=np.float32)
    for t in range(T):
        rows, want = _unfused_cycle(refs, b, actor, _slots(LEFT), zeros3, zeros2)
        _same(see[t], rows, f'see rows cycle {t}')
        _same(idx[t][:, :11], want, f'net_index cycle {t}')
    _same_engine(a, b, f'n={n}')
    assert (a.neck[:, :11] != 0).any() and not a.neck[:, 11:].any()      # the scripted team never turns its necks
    assert not a.neck[:, 22:].any() and (a.view_width[:, 22:] == 2).all() and not a.see_wait[:, 22:].any()   # pad slots untouched
    a.close(); b.close()


def test_done_and_red_cards(refs):
    """matches end inside the run (short halves, no extra time, no shoot-out, auto-reset); slots 3 and 15 sent off before it"""
    kw = dict(noise=True, seed=11, half_time_cycles=8, nr_extra_halfs=0, penalty_shoot_outs=0)
    n, off = 16, [3, 15]
    eng, orc = _pair(n, **kw)
    eng.enable_vision()
    actor = _actor(16, 16, 8, eps=0.2, seed=7)
    eng.set_network(actor, ALL)
    eng.reset(); orc.reset()
    eng.card[:, off] = 2
    snap = orc.snapshot()
    snap['card'][:, off] = 2
    orc.load(snap)
    seen = dict(finished=0, red_cycles=0)

    def each_cycle(cycle, s, see, before, after, done):
        d = done.astype(bool)
        seen['finished'] += int(d.sum())
        # the done cycle: neck +0, normal width, wait 0 -- and the timer of the same step makes it fresh (wait = 2)
        for k, v in (('neck', 0), ('view_width', 2), ('see_wait', 2)):
            assert (_bits(after[k][d][:, :22]) == v).all(), (cycle, k)
        red = s['card'][:, off] >= 2                         # (start of the cycle; a restarted match has its players back)
        seen['red_cycles'] += int(red.sum())
        rows = see[:, off]
        assert not _bits(rows[..., 16:21])[red].any() and not _bits(rows[..., 24:])[red].any()   # ball and player words +0
        still = red & ~d[:, None]                            # sent off, the match goes on: the three words stand
        for k in S.VISION_PLANES:
            assert np.array_equal(_bits(before[k][:, off])[still], _bits(after[k][:, off])[still]), (cycle, k)

    _closed_loop(refs, eng, orc, actor, ALL, ALL, 14, 2, each_cycle)
    assert seen['finished'] > 0 and seen['red_cycles'] > 0
    eng.close()


def test_other_slots_and_view_actions(refs):
    """the network on slots 1 and 12, the rest external with view actions: NaN moments, out-of-range moments, junk codes; the
    caller's rows of the network slots, body and view, are NaN and never read"""
    from soccer2d_amd.match import MatchEngine
    n, T = 5, 8
    mask = (1 << 1) | (1 << 12)
    slots = _slots(mask)
    actor = _actor(16, 48, 6, eps=0.25, seed=9)
    rng = np.random.default_rng(4)
    acts = np.zeros((T, n, 22, 3), dtype=np.float32)
    acts[..., 0] = rng.integers(0, 5, (T, n, 22))
    acts[..., 1] = rng.uniform(-100, 100, (T, n, 22))
    acts[..., 2] = rng.uniform(-180, 180, (T, n, 22))
    view = np.zeros((T, n, 22, 2), dtype=np.float32)
    view[..., 0] = rng.uniform(-400, 400, (T, n, 22))       # beyond +-180: clamped
    view[..., 0][rng.random((T, n, 22)) < 0.1] = np.nan
    view[..., 1] = rng.choice(np.array([0, 1, 2, 3, 4, -1, 2.5, np.nan, np.inf], dtype=np.float32), (T, n, 22))
    a = MatchEngine(n, 'cuda:0', noise=True, seed=5)
    b = MatchEngine(n, 'cuda:0', noise=True, seed=5)
    for e in (a, b):
        e.enable_vision()
        e.reset()
    a.set_network(actor, mask)
    poisoned_a, poisoned_v = acts.copy(), view.copy()
    poisoned_a[:, :, slots] = np.nan
    poisoned_v[:, :, slots] = np.nan
    out = a.rollout(T, actions=torch.from_numpy(poisoned_a).cuda(), view_actions=torch.from_numpy(poisoned_v).cuda(),
                    record_actions=True, net_index=True, see_obs=mask, with_obs=False)
    see, idx, rec = out['see'].cpu().numpy(), out['net_index'].cpu().numpy(), out['actions'].cpu().numpy()
    assert not np.isnan(rec[:, :, slots]).any()
    others = [i for i in range(22) if i not in slots]
    _same(rec[:, :, others], acts[:, :, others], 'caller rows in the record')
    for t in range(T):
        rows, want = _unfused_cycle(refs, b, actor, slots, acts[t], view[t])
        _same(see[t], rows[:, slots], f'see rows cycle {t}')
        _same(idx[t][:, slots], want, f'net_index cycle {t}')
    _same_engine(a, b, 'other slots')
    assert len(np.unique(a.view_width[:, :22].cpu().numpy())) == 3
    a.close(); b.close()


def test_record_only(refs):
    """no network, see_obs='left', the random policy: the record is the per-cycle see('left') of an unfused twin, the engine
    state that of a plain rollout, and the engine runs its old kernels afterwards"""
    from soccer2d_amd.match import MatchEngine
    n, T = 11, 6
    a, b, c = (MatchEngine(n, 'cuda:0', noise=True, seed=31) for _ in range(3))
    for e in (a, c):
        e.enable_vision()
    for e in (a, b, c):
        e.reset()
    name = a.kernel_name()
    out = a.rollout(T, see_obs='left', net_index=True, with_obs=False)
    assert out['see'].shape == (T, n, 11, 192) and (out['net_index'] == -1).all()
    assert a.kernel_name() == name and 'see network' not in name
    b.rollout(T, with_obs=False)
    torch.cuda.synchronize()
    assert torch.equal(a.arena, b.arena)
    for t in range(T):
        assert torch.equal(out['see'][t], c.see('left')), t
        c.rollout(1, with_obs=False)
        c.vision_step(None, done=True)
    _same_engine(a, c, 'record only')
    assert (a.see_wait[:, :22] > 0).all()
    a.close(); b.close(); c.close()


@pytest.mark.parametrize('h1', [16, 32, 48, 64])
@pytest.mark.parametrize('h2', [16, 32, 48, 64])
def test_shapes(refs, h1, h2):
    from soccer2d_amd.match import MatchEngine
    L, ML, SL = refs
    n, T = 2, 2
    for k in (1, 17, 64):
        eng = MatchEngine(n, 'cuda:0', noise=True, seed=h1 + h2 + k)
        eng.enable_vision()
        actor = _actor(h1, h2, k, eps=0.0, seed=h1 * 100 + h2 + k)
        eng.set_network(actor, ALL)
        eng.reset()
        out = eng.rollout(T, net_index=True, see_obs='all', with_obs=False)
        rows, idx = out['see'].cpu().numpy(), out['net_index'].cpu().numpy()
        want = MN.argmax(ML, SN.forward(L, rows, actor.params.cpu().numpy(), h1, h2, k))
        _same(idx, want, f'index {h1}-{h2}-{k}')
        eng.close()


def test_exploration_greedy_and_counter_wrap(refs):
    from soccer2d_amd.match import MatchEngine
    L, ML, SL = refs
    n, T, k = 64, 4, 5
    eng = MatchEngine(n, 'cuda:0', noise=True)
    eng.enable_vision()
    actor = _actor(16, 32, k, eps=1.0, seed=13)
    eng.set_network(actor)
    eng.reset()
    params = actor.params.cpu().numpy()
    # epsilon 1: exactly the host draws
    tick0 = eng.tick.cpu().numpy()
    idx = eng.rollout(T, net_index=True, with_obs=False)['net_index'].cpu().numpy()
    for t in range(T):
        wx, wy = MN.draws(eng.cfg.seed, np.arange(n), tick0 + t, range(22))
        _same(idx[t], ((wy.astype(np.uint64) * np.uint64(k)) >> np.uint64(32)).astype(np.int32), f'epsilon 1, cycle {t}')
    # epsilon 0: the greedy index of the recorded row
    actor.epsilon = 0.0
    out = eng.rollout(T, net_index=True, see_obs='all', with_obs=False)
    rows, idx = out['see'].cpu().numpy(), out['net_index'].cpu().numpy()
    _same(idx, MN.argmax(ML, SN.forward(L, rows, params, 16, 32, k)), 'epsilon 0')
    # the tick counter past 2^31 (the int32 view turns negative) and 2^32 (it wraps): the draws follow it
    actor.epsilon = 0.5
    start = np.array([2 ** 31 - 2, -2, 7], dtype=np.int32)[np.arange(n) % 3]
    eng.tick.copy_(torch.from_numpy(start))
    out = eng.rollout(T, net_index=True, see_obs='all', with_obs=False)
    rows, idx = out['see'].cpu().numpy(), out['net_index'].cpu().numpy()
    explored = 0
    for t in range(T):
        tick = (start.astype(np.int64) + t) & 0xFFFFFFFF
        want = SN.indices(L, ML, rows[t], params, 16, 32, k, 0.5, eng.cfg.seed, np.arange(n), tick, range(22))
        _same(idx[t], want, f'wrap cycle {t}')
        explored += int((want != MN.argmax(ML, SN.forward(L, rows[t], params, 16, 32, k))).sum())
    assert explored > 0
    eng.close()


def test_graph_replay_acts_with_new_weights_epsilon_and_table(refs):
    from soccer2d_amd.match import MatchEngine
    n, T = 64, 4
    actor = _actor(32, 32, 6, eps=0.3, seed=17)
    module = actor._module
    a = MatchEngine(n, 'cuda:0', noise=True)
    b = MatchEngine(n, 'cuda:0', noise=True)
    for e in (a, b):
        e.enable_vision()
        e.set_network(actor)
        e.reset()
    out = a.alloc_rollout(T, with_obs=False, record_actions=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.rollout(T, out=out, record_actions=True, net_index=True, see_obs='all', with_obs=False)
    torch.cuda.current_stream().wait_stream(s)
    b.rollout(T, record_actions=True, with_obs=False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                             # a plain linear capture: the pack kernel, then the cycle kernel
        a.rollout(T, out=out, record_actions=True, net_index=True, see_obs='all', with_obs=False)
    first = out['net_index'].clone()
    with torch.no_grad():
        for p in module.parameters():
            p.add_(torch.randn_like(p) * 0.5)
    actor.sync()
    actor.epsilon = 0.0
    actor.set_table(_table(6, 99))
    g.replay()
    ob = b.rollout(T, record_actions=True, net_index=True, see_obs='all', with_obs=False)
    torch.cuda.synchronize()
    for k in ('net_index', 'actions', 'see'):
        assert torch.equal(out[k], ob[k]), k
    _same_engine(a, b, 'after the replay')
    assert not torch.equal(first, out['net_index'])
    L, ML, SL = refs
    idx = out['net_index'].cpu().numpy()
    _same(idx, MN.argmax(ML, SN.forward(L, out['see'].cpu().numpy(), actor.params.cpu().numpy(), 32, 32, 6)), 'new weights, epsilon 0')
    _same(out['actions'].cpu().numpy(), actor.table.cpu().numpy()[idx][..., :3], 'new table')
    a.close(); b.close()


def test_rejections_leave_the_engine_unchanged():
    import ctypes as C
    from soccer2d_amd import _capi_match as M
    from soccer2d_amd.actor import MatchQNetActor
    from soccer2d_amd.match import MatchEngine
    n = 8
    eng = MatchEngine(n, 'cuda:0', noise=True)
    twin = MatchEngine(n, 'cuda:0', noise=True)
    actor = _actor(32, 32, 8, eps=0.1, seed=21)
    with pytest.raises(RuntimeError):
        eng.set_network(actor, 'left')                    # before enable_vision()
    assert eng.network is None and not eng.kernel_name().endswith('network>')
    for e in (eng, twin):
        e.enable_vision()
        e.set_network(actor, 'left')
        e.reset()
    name = eng.kernel_name()
    assert name.endswith('see network>')
    good = actor.c_struct(LEFT, eng.vision_params, eng.vision)

    def variant(**kw):
        s = M.S2DMatchSeeNet.from_buffer_copy(good)
        for f, v in kw.items():
            if f.startswith('prm_'):
                setattr(s.prm, f[4:], v)
            elif f.startswith('vis_'):
                setattr(s.vis, f[4:], v)
            else:
                setattr(s, f, v)
        return s
    bad = [variant(h1=24), variant(h2=80), variant(h1=0, slot_mask=0), variant(n_actions=0), variant(n_actions=65),
           variant(slot_mask=1 << 22), variant(params=actor.params.data_ptr() + 4), variant(params=None), variant(epsilon=None),
           variant(epsilon=actor.epsilon_tensor.data_ptr() + 2), variant(table=actor.table.data_ptr() + 2), variant(table=None),
           variant(vis_neck=None), variant(vis_view_width=None), variant(vis_see_wait=eng.see_wait.data_ptr() + 1),
           variant(vis_neck=eng.neck.data_ptr() + 2), variant(prm_visible_distance=-1.0), variant(prm_dist_round=0.0),
           variant(prm_min_neck_angle=100.0), variant(prm_unum_far_length=float('nan'))]
    s = variant()
    s.prm.see_interval[1] = 2.5
    bad.append(s)
    for s in bad:
        assert eng.lib.s2d_match_set_see_network(eng._h, C.byref(s)) != 0
    assert eng.kernel_name() == name
    # the see network is still the one set before the rejected calls: the next rollout is the twin's
    oa = eng.rollout(3, net_index=True, see_obs='all', record_actions=True, with_obs=False)
    ob = twin.rollout(3, net_index=True, see_obs='all', record_actions=True, with_obs=False)
    for k in ('net_index', 'see', 'actions'):
        assert torch.equal(oa[k], ob[k]), k
    _same_engine(eng, twin, 'after the rejections')
    assert (oa['net_index'][:, :, :11] >= 0).all() and (oa['net_index'][:, :, 11:] == -1).all()
    # a record-only struct (slot_mask 0) needs no network pointers
    assert eng.lib.s2d_match_set_see_network(eng._h, C.byref(variant(slot_mask=0, params=None, epsilon=None, table=None))) == 0
    assert eng.kernel_name().endswith('see network>')
    assert eng.lib.s2d_match_set_see_network(eng._h, C.byref(good)) == 0
    st, ro = eng._stream(), M.S2DMatchRollout()
    buf = torch.empty((1, n, 11, 224), device='cuda:0')
    # rollout_net with a see network set; rollout_see's own argument checks; rollout_see without a see network
    assert eng.lib.s2d_match_rollout_net(eng._h, 1, None, C.byref(ro), None, None, 0, None, st) != 0
    with pytest.raises(ValueError):
        eng.rollout(1, agent_obs='left', see_obs='left')
    assert eng.lib.s2d_match_rollout_see(eng._h, 1, None, None, C.byref(ro), None, None, 0, C.c_void_p(buf.data_ptr()), st) != 0
    assert eng.lib.s2d_match_rollout_see(eng._h, 1, None, None, C.byref(ro), None, None, 1 << 22, C.c_void_p(buf.data_ptr()), st) != 0
    assert eng.lib.s2d_match_rollout_see(eng._h, 1, None, None, C.byref(ro), None, None, LEFT, C.c_void_p(buf.data_ptr() + 4), st) != 0
    assert eng.lib.s2d_match_rollout_see(eng._h, 1, None, C.c_void_p(buf.data_ptr() + 2), C.byref(ro), None, None, 0, None, st) != 0
    torch.cuda.synchronize()
    _same_engine(eng, twin, 'after the rejected launches')
    # setting a 224-input network clears the see network, and the reverse; None clears either
    torch.manual_seed(1)
    m224 = torch.nn.Sequential(torch.nn.Linear(224, 16), torch.nn.ReLU(), torch.nn.Linear(16, 16), torch.nn.ReLU(),
                               torch.nn.Linear(16, 4)).to('cuda:0')
    agent = MatchQNetActor.from_module(m224, np.zeros((4, 3), dtype=np.float32))
    eng.set_network(agent, 'left')
    assert eng.kernel_name().endswith('network>') and not eng.kernel_name().endswith('see network>')
    assert eng.lib.s2d_match_rollout_see(eng._h, 1, None, None, C.byref(ro), None, None, 0, None, st) != 0
    with pytest.raises(ValueError):
        eng.rollout(1, see_obs='left')                    # a record-only launch would replace the agent-row network
    assert eng.rollout(1, net_index=True, agent_obs='left', with_obs=False)['agent_obs'].shape == (1, n, 11, 224)
    eng.set_network(actor, 'right')
    assert eng.kernel_name().endswith('see network>')
    assert eng.lib.s2d_match_rollout_net(eng._h, 1, None, C.byref(ro), None, None, 0, None, st) != 0
    eng.set_network(None)
    assert not eng.kernel_name().endswith('network>')
    with pytest.raises(ValueError):
        eng.rollout(1, view_actions=torch.zeros((1, n, 22, 3), device='cuda:0'))
    eng.close(); twin.close()


def test_vec_env_see_opponent():
    """the vec env's plumbing: shapes, the right team on the see actor, the left team's five action words split into body and view
    rows, no vision_step of its own -- against an engine driven by hand through the same fused launch (fused against unfused is
    the other tests')"""
    from soccer2d_amd.match import MatchEngine, Soccer2DMatchVecEnv
    n = 4
    kw = dict(noise=True, seed=41)
    actor = _actor(32, 32, 8, eps=0.0, seed=31)
    env = Soccer2DMatchVecEnv(n, opponent=actor, obs='see', **kw)
    assert env.observation_space.shape == (11, 192) and env.action_space.shape == (11, 5)
    assert env.engine.kernel_name().endswith('see network>') and env.engine.network_mask == 0x3FF800
    hand = MatchEngine(n, 'cuda:0', **kw)
    hand.set_controllers({'left': 'external', 'right': 'random'})
    hand.enable_vision()
    hand.set_network(actor, 'right')
    obs = env.reset()
    hand.reset()
    assert obs.shape == (n, 11, 192) and torch.equal(obs, hand.see('left'))
    g = torch.Generator(device='cuda:0').manual_seed(4)
    for t in range(8):
        a = torch.empty((n, 11, 5), device='cuda:0')
        a[..., 0] = torch.randint(0, 5, (n, 11), device='cuda:0', generator=g).float()
        a[..., 1] = torch.rand((n, 11), device='cuda:0', generator=g) * 200 - 100
        a[..., 2] = torch.rand((n, 11), device='cuda:0', generator=g) * 360 - 180
        a[..., 3] = torch.rand((n, 11), device='cuda:0', generator=g) * 120 - 60
        a[..., 4] = torch.randint(0, 4, (n, 11), device='cuda:0', generator=g).float()
        obs, rew, done, info = env.step(a)
        assert obs.shape == (n, 11, 192) and rew.shape == (n, 11)
        acts = torch.zeros((1, n, 22, 3), device='cuda:0')
        view = torch.zeros((1, n, 22, 2), device='cuda:0')
        acts[0, :, :11], view[0, :, :11] = a[..., :3], a[..., 3:]
        hand.rollout(1, actions=acts, view_actions=view, with_obs=False)   # one launch: no vision_step by hand either
        assert torch.equal(obs, hand.see('left')) and torch.equal(done, hand.done)
        _same_engine(env.engine, hand, f'step {t}')
    assert (env.engine.neck[:, 11:22] != 0).any()          # the right team's necks move as the table says
    assert (actor.table[:, 3] != 0).all()
    env.close(); hand.close()
    with pytest.raises(ValueError):
        Soccer2DMatchVecEnv(n, opponent=actor, obs='agent')


def test_enable_vision_again_with_a_see_network_set(refs):
    """a second enable_vision() (new planes, other parameters) while a see network is set: the engine follows -- the launch steps
    the NEW planes with the NEW parameters, as an unfused twin that enabled them once does"""
    from soccer2d_amd.match import MatchEngine
    n, T = 5, 8
    over = dict(view_angle=(40.0, 100.0, 170.0), see_interval=(1.0, 3.0, 4.0), max_neck_angle=60.0)
    actor = _actor(16, 16, 7, eps=0.0, seed=19)
    a = MatchEngine(n, 'cuda:0', noise=True, seed=61)
    b = MatchEngine(n, 'cuda:0', noise=True, seed=61)
    a.enable_vision()
    a.set_network(actor, 'all')
    old = (a.neck, a.view_width, a.see_wait)
    a.enable_vision(**over)
    assert a.kernel_name().endswith('see network>') and a.neck.data_ptr() != old[0].data_ptr()
    before = [t.clone() for t in old]
    b.enable_vision(**over)
    a.reset(); b.reset()
    out = a.rollout(T, net_index=True, see_obs='all', with_obs=False)
    see, idx = out['see'].cpu().numpy(), out['net_index'].cpu().numpy()
    zeros3, zeros2 = np.zeros((n, 22, 3), dtype=np.float32), np.zeros((n, 22, 2), dtype=np.float32)
    for t in range(T):
        rows, want = _unfused_cycle(refs, b, actor, _slots(ALL), zeros3, zeros2)
        _same(see[t], rows, f'see rows cycle {t}')
        _same(idx[t], want, f'net_index cycle {t}')
    _same_engine(a, b, 'second enable_vision')
    assert torch.equal(a.see('all'), b.see('all'))
    assert (a.neck[:, :22] != 0).any() and float(a.neck.max()) == 60.0        # the new upper neck limit
    for t, c in zip(old, before):                         # the first planes are no longer the engine's: nothing wrote them
        assert torch.equal(t, c)
    a.close(); b.close()
