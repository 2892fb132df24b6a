"""The belief layer on the GPU (s2d_match_belief_scan, s2d_match_belief_reset; include/s2d_match.h, "Belief"): bit-exact to the host
restatement (tests/belief_ref.c) fed the same see rows -- in a closed loop with the engine under every kind of slot mask, as a scan
against single steps, replayed from a captured graph, scanned over a fused rollout's see record against the per-cycle steps -- and
Soccer2DMatchVecEnv(obs='belief')."""
import numpy as np
import pytest

import belief as B
from soccer2d_amd import _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
SHORT = dict(noise=True, half_time_cycles=10, nr_extra_halfs=0, penalty_shoot_outs=0, after_goal_wait=5)   # matches restart inside a run
SCRIPTED = {'left': 'scripted', 'right': 'scripted'}


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return B.build(tmp_path_factory.mktemp('belief_ref'))


def _engine(n, slots='all', belief=None, seed=5, **kw):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(n, 'cuda:0', seed=seed, **dict(SHORT, **kw))
    eng.set_controllers(SCRIPTED)
    eng.enable_vision()
    eng.enable_belief(slots, **(belief or {}))
    eng.reset()
    return eng


def _view_actions(g, n):
    v = torch.empty((n, 22, 2), device='cuda:0')
    v[..., 0] = torch.rand((n, 22), device='cuda:0', generator=g) * 180 - 90
    v[..., 1] = torch.randint(0, 4, (n, 22), device='cuda:0', generator=g).float() * (torch.rand((n, 22), device='cuda:0', generator=g) < 0.3)
    return v


def _cycle(eng, g):
    """one cycle of the engine and its vision state; the see rows of the belief's slots and the engine's done"""
    eng.step(None)
    eng.vision_step(_view_actions(g, eng.num_envs), done=True)
    return eng.see(eng.belief_slots), eng.done


def _same(got, want, tag):
    g, w = np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f'{tag}: {len(bad)} words differ; first at {tuple(bad[0])}: gpu={got[tuple(bad[0])]!r} '
                             f'host={want[tuple(bad[0])]!r}')


OTHER = dict(ball_decay=0.9, player_decay=0.5, view_angle=(50.0, 100.0, 170.0), match_dist=2.0, match_rate=0.05, ghost_margin=3.0,
             count_max=6.0)


@pytest.mark.parametrize('n,slots,belief', [(37, 'all', None), (37, 'left', OTHER), (37, 1 << 15, None), (1, 'all', None)])
def test_closed_loop_with_the_engine(ref, n, slots, belief):
    """48 cycles, noise on, scripted against scripted, random TurnNeck / ChangeView per cycle, halves of 10 cycles (matches end
    and restart inside the run): after every cycle the device belief equals the restatement's on the same see rows"""
    eng = _engine(n, slots, belief)
    mask = M.agent_slot_mask(slots)
    k = B.popcount(mask)
    prm = B.params(**(belief or {}))
    assert tuple(eng.belief.shape) == (n, k, 192)
    host = eng.belief.cpu().numpy()
    _same(host, B.unknown(n, k), 'reset')
    g = torch.Generator(device='cuda:0').manual_seed(17)
    restarts = aged = matched = forgotten = 0
    for t in range(48):
        see, done = _cycle(eng, g)
        got = eng.belief_step(see, done=True)
        assert got is eng.belief
        d = done.cpu().numpy()
        before = host
        host = B.step(ref, prm, see.cpu().numpy(), host, d, mask)
        _same(got.cpu().numpy(), host, f'cycle {t}')
        restarts += int(d.sum())
        pc = host[:, :, 29::8]
        aged += int(((pc > 0) & (pc < prm.count_max)).sum())
        matched += int(((pc == 0) & (host[:, :, 30::8] > 0)).sum())      # placed by a level 1-3 sighting: the second pass
        forgotten += int(((before[:, :, 29::8] < prm.count_max - 1) & (pc == prm.count_max) & (d[:, None, None] == 0)).sum())   # ghosts
    assert restarts > 0 and aged > 0                       # matches restarted; entries were remembered while unseen
    assert matched > 0 and forgotten > 0                   # the association and the ghost rule took part
    cm = np.float32(prm.count_max)
    assert (host[:, :, 29::8] < cm).any() and (host[:, :, 29::8] == cm).any() and (host[:, :, 20] < cm).any()
    assert np.array_equal(host[:, :, :16], see.cpu().numpy()[:, :, :16])
    # a masked reset leaves the masked matches' rows unknown and the others alone
    m = np.zeros(n, dtype=np.uint8)
    m[::2] = 1
    eng.reset(torch.from_numpy(m).cuda())
    _same(eng.belief.cpu().numpy(), B.reset(ref, host, m), 'masked reset')
    eng.close()


def _record(n, T, seed=9):
    """a played see record [T, n, 22, 192] with the engine's done per cycle"""
    eng = _engine(n, seed=seed)
    g = torch.Generator(device='cuda:0').manual_seed(seed)
    rows, dones = [], []
    for _ in range(T):
        see, done = _cycle(eng, g)
        rows.append(see.clone()); dones.append(done.clone())
    return eng, torch.stack(rows), torch.stack(dones)


def test_scan_against_steps(ref):
    T, n = 16, 9
    eng, see, done = _record(n, T)
    g = torch.Generator(device='cuda:0').manual_seed(1)
    reset = ((torch.rand((T, n), device='cuda:0', generator=g) < 0.1) | done.bool()).to(torch.uint8)
    assert reset.any() and not reset.all()
    eng.reset()
    steps = []
    for t in range(T):
        steps.append(eng.belief_step(see[t], done=reset[t]).clone())
    final = eng.belief.clone()
    eng.reset()
    out = eng.belief_scan(see, reset=reset, out=True)
    assert tuple(out.shape) == (T, n, 22, 192)
    assert torch.equal(out.view(torch.int32), torch.stack(steps).view(torch.int32))
    assert torch.equal(out[T - 1].view(torch.int32), eng.belief.view(torch.int32)) and torch.equal(eng.belief.view(torch.int32), final.view(torch.int32))
    eng.reset()                                            # without a record: the state alone
    assert eng.belief_scan(see, reset=reset) is eng.belief
    assert torch.equal(eng.belief.view(torch.int32), final.view(torch.int32))
    hfin, hrec = B.scan(ref, B.params(), see.cpu().numpy(), B.unknown(n, 22), reset.cpu().numpy())
    _same(out.cpu().numpy(), hrec, 'scan')
    _same(final.cpu().numpy(), hfin, 'final')
    with pytest.raises(ValueError):
        eng.belief_scan(see[:, :, :11].contiguous())
    with pytest.raises(ValueError):
        eng.belief_scan(see, out=see)                       # the record may not be the input
    with pytest.raises(ValueError):
        eng.belief_scan(see.double())
    eng.close()


def test_graph_replay():
    """a captured see + belief_step, replayed three times, equals three eager steps on an engine of the same seed"""
    n = 9
    a, b, w = _engine(n, seed=3), _engine(n, seed=3), _engine(n, seed=3)
    ga, gb = (torch.Generator(device='cuda:0').manual_seed(4) for _ in range(2))
    for _ in range(3):                                     # some history first, eagerly on both
        for eng, g in ((a, ga), (b, gb)):
            see, _done = _cycle(eng, g)
            eng.belief_step(see, done=True)
    rows = torch.empty((n, 22, 192), device='cuda:0')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # a warm-up outside the capture, on an engine of its own
        w.belief_step(w.see('all', out=torch.empty_like(rows)), done=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    before = a.belief.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                          # a plain linear capture: the see kernel, then the scan kernel
        a.belief_step(a.see('all', out=rows), done=True)
    torch.cuda.synchronize()
    assert torch.equal(a.belief.view(torch.int32), before.view(torch.int32))   # capturing ran nothing
    for i in range(3):
        a.step(None); a.vision_step(_view_actions(ga, n), done=True)
        graph.replay()
        see, _done = _cycle(b, gb)
        b.belief_step(see, done=True)
        torch.cuda.synchronize()
        assert torch.equal(rows.view(torch.int32), see.view(torch.int32)), i
        assert torch.equal(a.belief.view(torch.int32), b.belief.view(torch.int32)), i
    assert (a.belief[:, :, 29::8] < 1000).any()
    for eng in (a, b, w):
        eng.close()


def _see_actor():
    from soccer2d_amd.actor import MatchQNetActor
    table = [[M.MCMD_DASH, 60.0, 0.0, 20.0, 0.0], [M.MCMD_TURN, 30.0, 0.0, -20.0, 1.0], [M.MCMD_KICK, 50.0, 10.0, 0.0, 3.0]]
    return MatchQNetActor(16, 16, 3, epsilon=0.5, obs='see', table=table)


def _unknown_rows(rows):
    """every entry of these belief rows [.., 192] is unknown, as a reset leaves it"""
    cnt = torch.zeros(192, dtype=torch.bool, device=rows.device)
    cnt[20] = True
    for w in (29, 30, 31):
        cnt[w::8] = True
    return bool((rows[..., cnt] == M.BELIEF_COUNT_LIMIT).all()) and not bool(rows[..., ~cnt].any())


@pytest.mark.parametrize('opponent', [None, 'scripted', 'see actor'])
def test_env_mode(opponent):
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    n = 24
    opp = _see_actor() if opponent == 'see actor' else opponent
    agents = 22 if opp is None else 11
    env = Soccer2DMatchVecEnv(n, opponent=opp, obs='belief', seed=2, **dict(SHORT, half_time_cycles=6))
    assert env.observation_space.shape == (agents, 192) and env.action_space.shape == (agents, 5)
    obs = env.reset()
    assert obs.shape == (n, agents, 192) and _unknown_rows(obs)
    g = torch.Generator(device='cuda:0').manual_seed(6)
    restarted = 0
    for t in range(20):
        a = torch.empty((n, agents, 5), device='cuda:0')
        a[..., 0] = torch.randint(0, 5, (n, agents), device='cuda:0', generator=g).float()
        a[..., 1] = torch.rand((n, agents), device='cuda:0', generator=g) * 200 - 100
        a[..., 2] = torch.rand((n, agents), device='cuda:0', generator=g) * 360 - 180
        a[..., 3] = torch.rand((n, agents), device='cuda:0', generator=g) * 120 - 60
        a[..., 4] = torch.randint(0, 4, (n, agents), device='cuda:0', generator=g).float()
        obs, rew, done, info = env.step(a)
        assert obs.shape == (n, agents, 192) and rew.shape == (n, agents) and done.shape == (n,)
        see = env.engine.see(env._slots)
        assert torch.equal(obs[..., :16].view(torch.int32), see[..., :16].view(torch.int32))     # the self block is the see row's
        assert torch.equal(obs[..., 21:24].view(torch.int32), see[..., 21:24].view(torch.int32))
        if t == 0:                                         # everybody is fresh in the first cycle: something was taken in
            assert (obs[..., 8] == 1).all() and (obs[..., 29::8] == 0).any()
        d = done.bool()
        if d.any():                                        # a restarted match forgets: nothing is older than this cycle
            restarted += int(d.sum())
            cnt = obs[d][..., 29::8]
            assert ((cnt == 0) | (cnt == 1000)).all()
    assert restarted > 0
    assert ((obs[..., 29::8] > 0) & (obs[..., 29::8] < 1000)).any()       # remembered while unseen
    mask = torch.zeros(n, dtype=torch.uint8, device='cuda:0')
    mask[1::3] = 1
    keep = obs.clone()
    obs = env.reset(mask)
    assert _unknown_rows(obs[1::3])
    rest = (mask == 0)
    assert torch.equal(obs[rest].view(torch.int32), keep[rest].view(torch.int32)) and not _unknown_rows(obs[rest])
    env.close()


def test_surface_errors():
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(4, 'cuda:0')
    with pytest.raises(RuntimeError, match='enable_vision'):
        eng.enable_belief()
    eng.enable_vision(view_angle=(40.0, 80.0, 160.0))
    with pytest.raises(RuntimeError, match='enable_belief'):
        eng.belief_step()
    eng.enable_belief('right', count_max=50)
    assert tuple(eng.belief_params.view_angle) == (40.0, 80.0, 160.0) and eng.belief_params.count_max == 50
    assert eng.belief_params.ball_decay == eng.cfg.sp.ball_decay and eng.belief_params.player_decay == eng.cfg.sp.player_decay
    assert tuple(eng.belief.shape) == (4, 11, 192)
    eng.reset()
    eng.step(None); eng.vision_step()
    out = eng.belief_step()                                # see defaults to the belief's own slots
    assert out is eng.belief and torch.equal(out[..., :16], eng.see('right')[..., :16])
    with pytest.raises(ValueError):
        eng.belief_step(eng.see('all'))
    with pytest.raises(ValueError):
        eng.enable_belief(count_max=0)
    eng.close()


@pytest.mark.parametrize('slots', ['all', 'left'])
def test_record_path_equals_the_per_cycle_path(slots):
    """INTEGRATION.md section 5i's learner path: the beliefs scanned over a fused rollout's see record equal, bit for bit, the ones
    belief_step builds cycle by cycle (what Soccer2DMatchVecEnv(obs='belief') shows a policy).  out['see'][t] is the START-of-cycle
    row of cycle t and out['done'][t] the done of cycle t, so the row AFTER cycle t is out['see'][t + 1] and its reset flag is
    out['done'][t]."""
    n, T = 9, 24
    g = torch.Generator(device='cuda:0').manual_seed(12)
    view = torch.stack([_view_actions(g, n) for _ in range(T + 1)])
    a, online, b = (_engine(n, slots, seed=7) for _ in range(3))
    # A: per cycle.  `online` also takes in the row it sees before its first action, as an agent acting from its belief does
    held = [online.belief_step().clone()]
    beliefs, rows = [], []
    for t in range(T):
        for eng in (a, online):
            eng.step(None)
            eng.vision_step(view[t], done=True)
        rows.append(a.see(slots).clone())
        beliefs.append(a.belief_step(rows[-1], done=True).clone())
        held.append(online.belief_step(done=True).clone())
    # B: one fused rollout, then one scan
    out = b.rollout(T + 1, with_obs=False, see_obs=slots, view_actions=view)
    see, done = out['see'], out['done']
    assert done[:T].any() and not done[:T].all()           # matches restarted inside the record
    for t in range(T):
        assert torch.equal(see[t + 1].view(torch.int32), rows[t].view(torch.int32)), f'see row after cycle {t}'
    got = b.belief_scan(see[1:], reset=done[:T], out=True)
    assert torch.equal(got.view(torch.int32), torch.stack(beliefs).view(torch.int32))
    assert torch.equal(b.belief.view(torch.int32), a.belief.view(torch.int32))
    # the learner's form: from row 0, flags shifted by one row -> the belief an online agent holds when it chooses action t
    b.reset()
    flags = torch.cat([torch.zeros_like(done[:1]), done[:T]])
    got = b.belief_scan(see, reset=flags, out=True)
    assert tuple(got.shape) == (T + 1, n, B.popcount(M.agent_slot_mask(slots)), 192)
    assert torch.equal(got.view(torch.int32), torch.stack(held).view(torch.int32))
    assert (got[..., 29::8] < 1000).any() and (got[1:][done[:T].bool()][..., 29::8] == 1000).any()
    for eng in (a, online, b):
        eng.close()
