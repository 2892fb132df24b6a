"""The two reflections of tests/match_symmetry.py on the 11v11 match KERNEL, without the oracle in the loop.

* FLIP_Y, bitwise: two engines per scene of tests/match_scenes.py, the second loaded with flip_y of the first's state and driven with
  flip_y of its commands (for the random-policy scenes: of the commands the first engine recorded).  Per step every word of
  STATE_FIELDS; through s2d_match_rollout_ex between two placements every word of the record.  On the instantiation the configuration
  selects and, for stock scenes, on the general one.  The placements (PLACEMENTS of match_symmetry, and the resets by mask) are decided
  from the first engine's own states, on the device; there the engines may differ in x, y, body of the placed slots and in nothing
  else, and the second is loaded again.
* Driven play on the device only: 1024 matches x 200 cycles from scattered states, commands made with torch, compared on the device,
  one copy to the host at the end.  A match leaves at its first placement; at least 90 % of the match-cycles are compared.
* SWAP_X: swap_x of the states test_gpu_match_f64.py steps (bodies snapped) through one device cycle, judged by that file's rule
  and bounds against the fp64 oracle."""
import numpy as np
import pytest

import match_oracle as MO
import match_scenes as MS
import match_symmetry as SY
from soccer2d_amd import _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

DEV = 'cuda:0'
SCENES = [s for s in MS.SCENES if not s.cfg.get('noise')]
CASES = [(sc, g) for sc in SCENES for g in ((False, True) if MS.stock_accepts(sc) else (False,))]
FIELDS = MO.STATE_FIELDS


def _engine(cfg, n, state):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(n, DEV, cfg=cfg)
    _load(eng, state)
    return eng


def _load(eng, state, where=None):
    """write a state (tensors or arrays) into the engine's planes; where: bool [n], the matches to write"""
    for k in FIELDS:
        dst = getattr(eng, k)
        v = torch.as_tensor(state[k], device=DEV)
        if where is not None:
            v = torch.where(where.view((-1,) + (1,) * (dst.dim() - 1)), v, dst)
        dst.copy_(v)


def _state(eng):
    return {k: getattr(eng, k).clone() for k in FIELDS}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _differs(k, got, want):
    """the device twin of match_symmetry.differs: bool tensor of the words that are not bitwise equal (+-0 equal in a negated word)"""
    d = _bits(got) != _bits(want)
    if k in SY.NEGATED_Y:
        d = d & ~((got == 0) & (want == 0))
    return d


def _cycle_diff(before, after, got, cfg):
    """(int64 [len(FIELDS)] words that differ and no placement excuses, bool [n, 22] placed slots): the device twin of flip_y_cycle"""
    placed = SY.placed_slots(before, after, cfg)
    parked = placed & ~(after['card'][:, :22] < M.CARD_RED)
    want = SY.flip_y(after, 'state')
    counts = []
    for k in FIELDS:
        d = _differs(k, got[k], want[k])
        if d.dim() == 2:
            d = d[:, :23].clone()
            if k in SY.PLACED_WORDS:
                d[:, :22] &= ~placed
        elif k in ('nearest_left', 'nearest_right'):
            d = d & ~(parked[:, :11] if k == 'nearest_left' else parked[:, 11:]).any(dim=1)
        counts.append(d.sum())
    return torch.stack(counts), placed


def _first(counts):
    """'cycle t field: n words' of the first non-zero entry of a [T, fields] count matrix"""
    t, f = [int(v) for v in np.argwhere(counts)[0]]
    return f'cycle {t} {FIELDS[f]}: {int(counts[t, f])} words differ'


def _acts(a):
    return None if a is None else torch.as_tensor(a, device=DEV)


@pytest.mark.parametrize('sc,general', CASES, ids=[f"{sc.name}-{'general' if g else 'own'}" for sc, g in CASES])
def test_flip_y_scene_on_device(sc, general, monkeypatch):
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    else:
        monkeypatch.delenv('S2D_MATCH_GENERAL_KERNEL', raising=False)
    orc0 = MS.make_oracle(sc)                        # (only the scene's initial state comes from the oracle's setters)
    s0 = orc0.snapshot()
    cfg, cfg2 = orc0.cfg, SY.flip_y(orc0.cfg)
    e1, e2 = _engine(cfg, sc.n, s0), _engine(cfg2, sc.n, SY.flip_y(s0))
    name = e1.kernel_name()
    assert e2.kernel_name() == name and ('<general' in name) == (general or not MS.stock_accepts(sc)), name
    acts = _acts(MS.scene_actions(sc))

    # 1. per step: every word of the state
    counts, placed_at, used = [], [], []
    for t in range(sc.T):
        mask = MS.reset_mask(sc, t)
        if mask is not None:
            m = None if mask.all() else torch.as_tensor(mask, device=DEV)
            e1.reset(m); e2.reset(m)
            _load(e2, SY.flip_y(_state(e1), 'state'))                     # a reset by mask is a placement
        before = _state(e1)
        if acts is None:
            a = e1.rollout(1, None, with_obs=False, record_actions=True)['actions'][0]
        else:
            a = acts[t]
            e1.step(a)
        e2.step(SY.flip_y(a, 'actions'))
        after = _state(e1)
        c, placed = _cycle_diff(before, after, _state(e2), cfg)
        counts.append(c); placed_at.append(placed); used.append(a)
        _load(e2, SY.flip_y(after, 'state'), where=placed.any(dim=1))
    counts = torch.stack(counts).cpu().numpy()
    assert not counts.any(), f'{sc.name} [{name}] step: ' + _first(counts)
    assert torch.equal(e1.stats, e2.stats)
    placed_at = torch.stack(placed_at)                                    # [T, n, 22]
    cut_after = placed_at.flatten(1).any(dim=1).cpu().numpy()             # cycles that end in a placement

    # 2. s2d_match_rollout_ex with the record on: one launch between two placements (a placement cycle ends its launch)
    r1, r2 = _engine(cfg, sc.n, s0), _engine(cfg2, sc.n, SY.flip_y(s0))
    cuts = sorted({0, sc.T} | {t for t, _m in sc.resets} | {t + 1 for t in np.flatnonzero(cut_after)})
    bad = []
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        mask = MS.reset_mask(sc, t0)
        if mask is not None:
            m = None if mask.all() else torch.as_tensor(mask, device=DEV)
            r1.reset(m); r2.reset(m)
            _load(r2, SY.flip_y(_state(r1), 'state'))
        o1 = r1.rollout(t1 - t0, None if acts is None else acts[t0:t1], with_obs=True, record_actions=True)
        a2 = SY.flip_y(o1['actions'], 'actions')
        assert torch.equal(_bits(o1['actions']), _bits(torch.stack(used[t0:t1])))       # the commands of part 1 again
        o2 = r2.rollout(t1 - t0, a2, with_obs=True, record_actions=True)
        want = SY.flip_y({k: o1[k] for k in ('obs', 'mode', 'reward', 'done', 'actions')}, 'record')
        for k in ('mode', 'reward', 'done', 'actions'):
            bad.append((_bits(o2[k]) != _bits(want[k])).sum())
        for c, f in enumerate(('x', 'y', 'vx', 'vy', 'body')):
            d = _differs(f, o2['obs'][..., :23, c], want['obs'][..., :23, c]).clone()
            if f in SY.PLACED_WORDS:
                d[-1, :, :22] &= ~placed_at[t1 - 1]                       # (only the launch's last cycle can be a placement)
            bad.append(d.sum())
        _load(r2, SY.flip_y(_state(r1), 'state'), where=placed_at[t1 - 1].any(dim=1))
    final = [_differs(k, getattr(r2, k), SY.flip_y(_state(r1), 'state')[k]).sum() for k in FIELDS]
    assert torch.equal(r1.stats, r2.stats) and torch.equal(r1.stats, e1.stats)
    bad = torch.stack(bad).cpu().numpy().reshape(len(cuts) - 1, 9)
    assert not bad.any(), f'{sc.name} [{name}] record: launch {np.argwhere(bad)[0][0]} of {len(cuts) - 1}, word ' \
                          f"{('mode', 'reward', 'done', 'actions', 'x', 'y', 'vx', 'vy', 'body')[np.argwhere(bad)[0][1]]}"
    assert not torch.stack(final).cpu().numpy().any()
    for k in FIELDS:                                                       # the two entry points agree (first engines)
        assert torch.equal(_bits(getattr(r1, k)), _bits(getattr(e1, k))), k


# ------------------------------------------------------------------ driven play, on the device only
DRIVEN_N, DRIVEN_T = 1024, 200


def _driven_commands(g, s):
    """float32 [n, 22, 3] made on the device: all six commands; a player at the ball mostly kicks or tackles, a goalie near it mostly
    catches, two thirds of the others turn to the ball and dash (the device twin of match_symmetry.driven_commands)"""
    n = s['x'].shape[0]
    rnd = lambda: torch.rand((n, 22), generator=g, device=DEV)
    dx, dy = s['x'][:, 22:23] - s['x'][:, :22], s['y'][:, 22:23] - s['y'][:, :22]
    d = torch.hypot(dx, dy)
    u, v = rnd(), rnd()
    cmd = torch.full((n, 22), float(M.MCMD_NONE), device=DEV)
    for bound, c in ((0.88, M.MCMD_MOVE), (0.83, M.MCMD_CATCH), (0.78, M.MCMD_TACKLE), (0.75, M.MCMD_KICK), (0.65, M.MCMD_TURN),
                     (0.45, M.MCMD_DASH)):
        cmd = torch.where(u < bound, torch.full_like(cmd, float(c)), cmd)
    cmd = torch.where((d < 1.3) & (v < 0.6), torch.full_like(cmd, float(M.MCMD_KICK)), cmd)
    cmd = torch.where((d < 2.2) & (v >= 0.6) & (v < 0.75), torch.full_like(cmd, float(M.MCMD_TACKLE)), cmd)
    goalie = torch.zeros((n, 22), dtype=torch.bool, device=DEV)
    goalie[:, [0, 11]] = True
    cmd = torch.where(goalie & (d < 2.0) & (v < 0.5), torch.full_like(cmd, float(M.MCMD_CATCH)), cmd)
    power, ang = rnd() * 100.0, rnd() * 360.0 - 180.0
    two = (cmd == M.MCMD_DASH) | (cmd == M.MCMD_KICK)
    a1, a2 = torch.where(two, power, ang), torch.where(two, ang, torch.zeros_like(ang))
    a2 = torch.where((cmd == M.MCMD_TACKLE) & (rnd() < 0.15), torch.ones_like(a2), a2)
    mv = cmd == M.MCMD_MOVE
    a1, a2 = torch.where(mv, rnd() * -52.0, a1), torch.where(mv, rnd() * 68.0 - 34.0, a2)
    a1 = torch.where(cmd == M.MCMD_CATCH, rnd() * 120.0 - 60.0, a1)
    to_ball = torch.rad2deg(torch.atan2(dy, dx)) - s['body'][:, :22]
    to_ball = torch.remainder(to_ball + 180.0, 360.0) - 180.0
    free = (cmd == M.MCMD_DASH) | (cmd == M.MCMD_TURN) | (cmd == M.MCMD_NONE) | mv
    chase = (rnd() < 0.66) & free & (d >= 1.3)
    turn = chase & (to_ball.abs() > 12.0)
    cmd = torch.where(chase, torch.where(turn, torch.full_like(cmd, float(M.MCMD_TURN)), torch.full_like(cmd, float(M.MCMD_DASH))), cmd)
    a1 = torch.where(chase, torch.where(turn, to_ball, torch.full_like(a1, 100.0)), a1)
    a2 = torch.where(chase, torch.zeros_like(a2), a2)
    return torch.stack([cmd, a1, a2], dim=-1).contiguous()


@pytest.mark.parametrize('general', [False, True], ids=['stock', 'general'])
def test_flip_y_driven_play_on_device(general, monkeypatch):
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    else:
        monkeypatch.delenv('S2D_MATCH_GENERAL_KERNEL', raising=False)
    cfg = SY.driven_config()
    s0 = SY.scattered_state(cfg, DRIVEN_N, 2207)
    e1, e2 = _engine(cfg, DRIVEN_N, s0), _engine(SY.flip_y(cfg), DRIVEN_N, SY.flip_y(s0))
    want = 's2d_match_rollout_kernel<general>' if general else 's2d_match_rollout_kernel<stock>'     # heterogeneous types, stock rules
    assert e1.kernel_name() == e2.kernel_name() == want, e1.kernel_name()
    g = torch.Generator(device=DEV).manual_seed(5)
    paired = torch.ones(DRIVEN_N, dtype=torch.bool, device=DEV)
    compared = torch.zeros((), dtype=torch.int64, device=DEV)
    different = torch.zeros(len(FIELDS), dtype=torch.int64, device=DEV)
    commands = torch.zeros(7, dtype=torch.int64, device=DEV)
    for _t in range(DRIVEN_T):
        before = _state(e1)
        a = _driven_commands(g, before)
        commands += (a[..., 0].flatten()[:, None] == torch.arange(7, device=DEV)).sum(dim=0)
        e1.step(a); e2.step(SY.flip_y(a, 'actions'))
        after, got = _state(e1), _state(e2)
        paired &= ~SY.placed_slots(before, after, cfg).any(dim=1)          # a match leaves at its first placement
        want = SY.flip_y(after, 'state')
        compared += paired.sum()
        different += torch.stack([((_differs(k, got[k], want[k])[:, :23].any(dim=1) if got[k].dim() == 2
                                    else _differs(k, got[k], want[k])) & paired).sum() for k in FIELDS])
    out = torch.cat([compared.view(1), different, commands, e1.stats]).cpu().numpy()      # the one copy to the host
    compared, different, commands, stats = int(out[0]), out[1:1 + len(FIELDS)], out[1 + len(FIELDS):8 + len(FIELDS)], out[8 + len(FIELDS):]
    print(f'driven play on the device: compared {compared} of {DRIVEN_N * DRIVEN_T} match-cycles, commands {list(commands)}, stats {list(stats)}')
    assert not different.any(), {k: int(v) for k, v in zip(FIELDS, different) if v}
    assert compared >= 0.9 * DRIVEN_N * DRIVEN_T, compared
    assert (commands > 0).all() and stats[4] > 1000 and stats[5] > 300, (list(commands), list(stats))


# ------------------------------------------------------------------ SWAP_X through the fp64 rule of tests/test_gpu_match_f64.py
SWAP_N = 1024


def _swapped_kw(kw):
    kw = dict(kw)
    if kw.get('player_type_id') is not None:
        kw['player_type_id'] = [kw['player_type_id'][i] for i in SY.PERM[:22]]
    return kw


@pytest.mark.parametrize('k', range(5), ids=['stock, stock types', 'stock', 'stock rules, own schedule', 'general',
                                             'general, illegal defense'])
def test_swap_x_of_the_f64_corpus_states_matches_f64(k):
    """the states test_kernel_one_cycle_matches_f64 steps, swapped: one device cycle each, by match_f64's rule and bounds"""
    import test_gpu_match_f64 as TF
    name, kw, ends = TF.KERNELS[k]
    eng, _ocfg = TF._engines(SWAP_N, **dict(kw))
    swapped, ocfg2 = TF._engines(SWAP_N, **_swapped_kw(kw))
    assert eng.kernel_name() == swapped.kernel_name() == f's2d_match_rollout_kernel<{name}>'
    g = torch.Generator(device='cpu').manual_seed(11)
    end = torch.tensor(ends, dtype=torch.int32)[torch.randint(0, len(ends), (SWAP_N,), generator=g)]
    lead = torch.randint(1, 12 if ends[1] > 100 else 4, (SWAP_N,), generator=g, dtype=torch.int32)
    eng.cycle.copy_((end - lead).clamp(min=0).to(eng.device))
    modes, done = set(), 0
    for c in TF.CHECKPOINTS:
        if c > done:
            eng.rollout(c - done, with_obs=False)
        done = c
        s = SY.swap_x(SY.snap_bodies(TF._device_state(eng)))
        TF._write_state(swapped, s)
        m, _ev = TF._one_cycle(swapped, ocfg2, tag=f'swap_x of {name} cycle {c}')
        modes |= m
    assert {M.GM_PLAY_ON, M.GM_KICK_OFF} <= modes and TF.SHOOT_OUT & modes, sorted(modes)
