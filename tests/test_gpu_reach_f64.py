"""The reach-ball KERNELS against the fp64 libm build of the oracle.  States are written into the engine through its state views
(episode and policy_step included, so resets and draws line up), one launch runs, the state is read back; every case asserts, in
this order: (1) the device is bitwise the fp32 oracle's from the same written state -- which says which side is wrong if the next
step fails --, (2) the rule of tests/reach_f64.py holds for the device's words against float64 under the T values measured on the
host corpus (tests/test_reach_oracle_f64.py), (3) the ill-conditioned share is at most 1 %.  Entry points: s2d_step with every
action kind and S2D_ACT_COMMAND, s2d_step_k, one-cycle and three-cycle rollouts through the unified kernel, the four-wave pipeline
and the two-envs-per-lane pipeline, the fused actors at epsilon = 1, s2d_reset.  512 envs per case: 8 groups of the four-wave
pipeline, 4 of the two-envs-per-lane one, 2 blocks of the step kernel."""
import numpy as np
import pytest

import oracle as O
import reach_f64 as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

N = 512
FAMILIES = {'unified': (dict(S2D_ROLLOUT_WS='0', S2D_ROLLOUT_E='1'), 's2d_reach_rollout_kernel<'),
            'ws': (dict(S2D_ROLLOUT_WS='1', S2D_ROLLOUT_E='1'), 's2d_reach_rollout_ws_kernel<'),
            'ws2': (dict(S2D_ROLLOUT_WS='1', S2D_ROLLOUT_E='2'), 's2d_reach_rollout_ws2_kernel')}
f32 = np.float32


def _engine(n, kw):
    from test_gpu_parity import _engine as make
    eng = make(n, **dict(kw))
    eng.reset()
    return eng


def _family(monkeypatch, family):
    for k, v in FAMILIES[family][0].items():
        monkeypatch.setenv(k, v)                            # read by s2d_create
    return FAMILIES[family][1]


def write_rows(eng, rows):
    for i, f in enumerate(R.F):
        t = getattr(eng, f)
        t.copy_(torch.as_tensor(rows[:, i].astype(f32 if i < R.NF else np.int32), device=t.device))
    torch.cuda.synchronize()


def read_out(eng):
    torch.cuda.synchronize()
    g = lambda t, dt: t.detach().cpu().numpy().astype(dt)
    return dict(state=np.stack([g(getattr(eng, f), np.float64) for f in R.F], axis=1), obs=g(eng.obs, np.float64),
                reward=g(eng.reward, np.float64), done=g(eng.done, np.int64), result=g(eng.result, np.int64),
                action_cmd=g(eng.action_cmd, np.int64), action_dir=g(eng.action_dir, np.float64),
                terminal_obs=g(eng.terminal_obs, np.float64))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(f32)).view(np.int32)


def assert_bitwise(dev, orc, cfg, tag, frozen=None, ended=None):
    """every state word and every output word of the device equals the fp32 oracle's (terminal_obs where the env ended with
    auto-reset on -- `ended`: in any cycle of a longer launch --; the outputs of a frozen env are not part of the cycle)"""
    n = len(dev['done'])
    live = np.ones(n, bool) if frozen is None else ~frozen
    for i, f in enumerate(R.F):
        a, b = (_bits(dev['state'][:, i]), _bits(orc['state'][:, i])) if i < R.NF else (dev['state'][:, i], orc['state'][:, i])
        bad = np.flatnonzero(a != b)
        assert not len(bad), f"{tag}: state.{f} differs in {len(bad)} envs; env {bad[0]}: device {dev['state'][bad[0], i]!r} oracle {orc['state'][bad[0], i]!r}"
    ended = ((orc['done'] != 0) if ended is None else ended) & bool(cfg.auto_reset)
    for w, use in (('done', live), ('result', live), ('action_cmd', live), ('reward', live), ('action_dir', live), ('obs', live),
                   ('terminal_obs', ended & live)):
        a, b = (dev[w], orc[w]) if w in ('done', 'result', 'action_cmd') else (_bits(dev[w]), _bits(orc[w]))
        d = a != b
        d = d.any(axis=1) if d.ndim == 2 else d
        bad = np.flatnonzero(d & use)
        assert not len(bad), f'{tag}: {w} differs in {len(bad)} envs; env {bad[0]}: device {dev[w][bad[0]]!r} oracle {orc[w][bad[0]]!r}'


def _frozen(actions, command):
    if not command:
        return None
    c = np.asarray(actions, dtype=f32)[:, 0]
    return (c >= -1.5) & (c <= -0.5)


def one_cycle(eng, cfg, rows, actions, command, launch, tag, cap=R.ILL_CAP):
    """write, launch one cycle, read back; bitwise against the fp32 oracle, the rule against float64, the ill-conditioned cap"""
    write_rows(eng, rows)
    launch(eng, actions)
    dev = read_out(eng)
    orc = R.f32_step(cfg, rows, actions, command)
    assert_bitwise(dev, orc, cfg, tag, _frozen(actions, command))
    dev['tries'] = orc['tries']                             # (the device equals the fp32 oracle: its resets drew as many candidates)
    rep, fails = R.compare(cfg, rows, actions, dev, command)
    print(f"{tag}: ill-conditioned {rep['ill']} of {rep['n']} {rep['ill_words']}, {rep['ended']} ended into a reset; worst "
          f"{ {w: round(v, 2) for w, v in rep['worst'].items() if v > 0} }")
    assert not fails, f'{tag}: ' + '\n'.join(fails[:10])
    if cap is not None:
        assert rep['ill'] <= cap * rep['n'], (tag, rep['ill'], rep['ill_words'])
    if rep['reset']:
        assert rep['reset']['skipped'] <= max(R.TRIES_CAP * rep['ended'], 0), (tag, rep['reset']['skipped'])
    return rep, dev


def _dev_actions(a, lead=False):
    t = torch.as_tensor(np.asarray(a), device='cuda:0')
    return t[None] if lead else t


def _step(eng, a):
    eng.step(_dev_actions(a))
    assert eng.kernel_name() == 's2d_reach_step_kernel'


def _step_commands(eng, a):
    eng.step_commands(_dev_actions(a))
    assert eng.kernel_name() == 's2d_reach_step_kernel'


def _trim(items):
    """about four time points of a host case (a subset of its batches: the host corpus measured T on every one of them)"""
    return items[::4] if len(items) > 8 else items[::2]


def rollout_from(eng, cfg, rows, acts, tag):
    """a launch of len(acts) cycles from the written state with caller actions [T, n, ...]: records, outputs and state bitwise the
    fp32 oracle's (the written states are entered mid-launch too; with auto-reset the prepared-episode slots serve the resets)"""
    write_rows(eng, rows)
    out = eng.rollout(len(acts), _dev_actions(acts))
    dev = read_out(eng)
    orc = O.OracleEngine(cfg, len(rows), 'f32')
    R.load_rows(orc, rows)
    ref = orc.rollout(len(acts), acts)
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        a, b = out[k].cpu().numpy(), ref[k]
        a, b = (a.view(np.int32), b.view(np.int32)) if a.dtype == f32 else (a, b)
        assert a.shape == b.shape and np.array_equal(a, b), f'{tag}: record {k} differs in {int((a != b).sum())} words'
    last = R.outputs(orc)
    orc.close()
    assert_bitwise(dev, last, cfg, tag, ended=ref['done'].any(axis=0))
    return ref


# ------------------------------------------------------------------------------------------------------------------------ s2d_step
@pytest.mark.parametrize('name', R.case_names())
def test_step_one_cycle(name):
    """s2d_step from the played and written corpora of the host test, about four batches per case, caller actions of every kind and
    S2D_ACT_COMMAND"""
    kw, command, items = R.build_case(name)
    cfg = R.make_cfg(kw)
    eng = _engine(N, kw)
    ended = 0
    for k, (rows, a) in enumerate(_trim(items)):
        if a.dtype == np.int64 and k % 2:                   # both discrete layouts of include/s2d.h
            a = a.astype(np.int32)
        rep, _ = one_cycle(eng, cfg, rows, a, command, _step_commands if command else _step, f'{name} batch {k}',
                           cap=R.ILL_CAP if R.capped(name) else None)
        ended += rep['ended']
    if name.startswith('written') and cfg.auto_reset:
        assert ended > 50                                   # resets inside the step, from written step numbers and positions


@pytest.mark.parametrize('k', [2, 4])
@pytest.mark.parametrize('name', ['written dqn-discrete16', 'written turning4', 'written noise-on', 'written no-autoreset-collide'])
def test_step_k(name, k):
    """s2d_step_k: every cycle's record, the last outputs and the state bitwise the fp32 oracle's; the first cycle's words under
    the rule"""
    kw, _, items = R.build_case(name)
    cfg = R.make_cfg(kw)
    eng = _engine(N, kw)
    rows, a0 = items[0]
    rs = np.random.RandomState(k)
    acts = np.stack([a0] + [R.random_actions(rs, cfg, N) for _ in range(k - 1)])
    write_rows(eng, rows)
    out = eng.step_k(k, _dev_actions(acts))
    assert eng.kernel_name() == 's2d_reach_step_k_kernel'
    dev = read_out(eng)
    orc = O.OracleEngine(cfg, N, 'f32')
    R.load_rows(orc, rows)
    ref = orc.rollout(k, acts)
    for w in ('obs', 'action', 'reward', 'done', 'result'):
        a, b = out[w].cpu().numpy(), ref[w]
        a, b = (a.view(np.int32), b.view(np.int32)) if a.dtype == f32 else (a, b)
        assert np.array_equal(a, b), f'{name} k={k}: record {w} differs in {int((a != b).sum())} words'
    last = R.outputs(orc)
    orc.close()
    assert_bitwise(dev, last, cfg, f'{name} k={k}', ended=ref['done'].any(axis=0))
    # the first cycle under the rule: the words the device recorded for it, and (the launch keeps no state between its cycles) the
    # fp32 oracle's state after one cycle, which the bitwise records of the later cycles were computed from
    first = R.f32_step(cfg, rows, a0)
    first.update({w: out[w][0].cpu().numpy().astype(np.float64 if w in ('obs', 'reward') else np.int64)
                  for w in ('obs', 'reward', 'done', 'result')})
    rep, fails = R.compare(cfg, rows, a0, first)
    assert not fails, '\n'.join(fails[:10])
    assert rep['ill'] <= R.ILL_CAP * N


# ------------------------------------------------------------------------------------------------------------------------ rollouts
ROLLOUT_CASES = ['written dqn-discrete16', 'written continuous1', 'written turning4', 'written noise-on', 'written random-server-1',
                 'written random-server-2', 'played no-autoreset-collide']


@pytest.mark.parametrize('family', list(FAMILIES))
@pytest.mark.parametrize('name', ROLLOUT_CASES)
def test_rollout_one_and_three_cycles(name, family, monkeypatch):
    """rollout(1) from written states through each kernel family (kernel_name asserted): bitwise, then the rule; rollout(3) from
    the same states: bitwise"""
    prefix = _family(monkeypatch, family)
    kw, _, items = R.build_case(name)
    cfg = R.make_cfg(kw)
    eng = _engine(N, kw)

    def launch(eng, a):
        eng.rollout(1, _dev_actions(a, lead=True))
        assert eng.kernel_name().startswith(prefix), eng.kernel_name()

    for k, (rows, a) in enumerate(_trim(items)[:2]):
        one_cycle(eng, cfg, rows, a, False, launch, f'{name} {family} batch {k}')
        rs = np.random.RandomState(100 + k)
        acts = np.stack([a] + [R.random_actions(rs, cfg, N) for _ in range(2)])
        rollout_from(eng, cfg, rows, acts, f'{name} {family} batch {k} T=3')
        assert eng.kernel_name().startswith(prefix), eng.kernel_name()


@pytest.mark.parametrize('noise', [False, True])
@pytest.mark.parametrize('family,n', [('unified', 64), ('ws', 64), ('ws', 128), ('ws2', 128)])
def test_dash_fast_path_groups(family, n, noise, monkeypatch):
    """groups whose envs all qualify for the dash fast path (stamina words on the table, whole-degree bodies) and sit on the speed
    clamps, the Goal and Out bounds, inside the collision radius and on the last steps of the episode: the table code sees them;
    the same group with one foreign env: the generic loop sees them.  rollout(1): bitwise and the rule; rollout(3): bitwise."""
    prefix = _family(monkeypatch, family)
    kw, items = R.fast_path_case(noise)
    cfg = R.make_cfg(kw)
    eng = _engine(n, kw)

    def launch(eng, a):
        eng.rollout(1, _dev_actions(a, lead=True))
        assert eng.kernel_name().startswith(prefix), eng.kernel_name()

    rows, a = items[0][0][:n], items[0][1][:n]
    tab = R.stamina_table(cfg)
    sn = rows[:, R.IDX['step_number']].astype(int)
    assert np.array_equal(rows[:, R.IDX['stamina']], tab[sn, 0]) and (rows[:, R.IDX['player_body']] == np.rint(rows[:, R.IDX['player_body']])).all()
    for foreign in (None, n - 3):
        r = rows.copy()
        if foreign is not None:
            r[foreign, R.IDX['stamina']] = float(f32(r[foreign, R.IDX['stamina']] - 123.25))
        tag = f'fast path {family} n={n} noise={noise} foreign={foreign}'
        rep, _ = one_cycle(eng, cfg, r, a, False, launch, tag, cap=None)
        assert rep['ill'] <= max(R.ILL_CAP * n, 1) and rep['ended'] > n // 8
        rs = np.random.RandomState(7)
        acts = np.stack([a] + [R.random_actions(rs, cfg, n) for _ in range(2)])
        ref = rollout_from(eng, cfg, r, acts, tag + ' T=3')
        assert ref['done'].sum() > n // 4


# ------------------------------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize('name', list(R.SCENE_CONFIGS))
def test_scenes_on_device(name):
    """every constructed scene through s2d_step (S2D_ACT_COMMAND, or the continuous action of the tie scenes): the device is bitwise
    the fp32 oracle's, gives the float64 discrete words in every scene not marked ill-conditioned, and obeys the rule where the
    probe leaves the scene well-conditioned"""
    items = [s for s in R.scenes() if s['cfg'] == name]
    cfg, rows, a, command = R.scene_batch(name, items)
    eng = _engine(len(items), R.SCENE_CONFIGS[name])
    rep, dev = one_cycle(eng, cfg, rows, a, command, _step_commands if command else _step, f'scenes {name}', cap=None)
    unit = R.units(cfg)
    fails = []
    for i, s in enumerate(items):
        fails += R.check_scene_f64(s, rep['f64'], i) + R.check_scene_f32(s, dev, rep['f64'], i, unit)
        if s['ill'] and not rep['ill_mask'][i]:
            fails.append(f"{s['name']}: the probe does not flag it ill-conditioned")
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('auto_reset', [False, True])
@pytest.mark.parametrize('family', list(FAMILIES))
def test_scene_states_through_the_rollout_kernels(family, auto_reset, monkeypatch):
    """the scenes' states (Goal, Out, Timeout, label overwrite, collisions, -0, clamps, stamina edges) entered by rollout(1) and
    mid-launch by rollout(3) in each kernel family, with discrete caller actions: bitwise the fp32 oracle's; the rule on rollout(1)"""
    prefix = _family(monkeypatch, family)
    kw, cfg, rows, a = R.scene_state_case(auto_reset)
    eng = _engine(N, kw)

    def launch(eng, acts):
        eng.rollout(1, _dev_actions(acts, lead=True))
        assert eng.kernel_name().startswith(prefix), eng.kernel_name()

    rep, _ = one_cycle(eng, cfg, rows, a, False, launch, f'scene states {family} auto_reset={auto_reset}', cap=None)
    assert rep['ended'] > 50 if auto_reset else rep['ended'] == 0
    acts = np.stack([a, (a + 5) % 16, (a + 11) % 16])
    ref = rollout_from(eng, cfg, rows, acts, f'scene states {family} auto_reset={auto_reset} T=3')
    assert eng.kernel_name().startswith(prefix) and ref['done'][0].sum() > 50


def test_scene_states_through_the_fused_qnet_actor():
    """s2d_rollout_qnet at epsilon = 1 is the random-policy rollout bit for bit: one launch from the written scene states against the
    fp32 oracle's random policy"""
    from soccer2d_amd.actor import QNetActor
    kw, cfg, rows, _ = R.scene_state_case(True)
    eng = _engine(N, kw)
    actor = QNetActor(64, 64, 16, device='cuda:0', epsilon=1.0)
    write_rows(eng, rows)
    out = eng.rollout_qnet(3, actor)
    assert eng.kernel_name().startswith('s2d_reach_qnet_rollout_kernel<'), eng.kernel_name()
    _against_random_policy(eng, cfg, rows, out, 3, 'qnet')


@pytest.mark.parametrize('name', ['written continuous1', 'written turning4'])
def test_written_states_through_the_fused_ddpg_actor(name):
    """s2d_rollout_actor at epsilon = 1, no action noise: the random-policy rollout from written states, continuous and turning"""
    from soccer2d_amd.actor import DeterministicActor
    kw, _, items = R.build_case(name)
    cfg = R.make_cfg(kw)
    eng = _engine(N, kw)
    actor = DeterministicActor(64, 64, 4 if cfg.task.use_turning else 1, device='cuda:0', epsilon=1.0)
    rows = items[0][0]
    write_rows(eng, rows)
    out = eng.rollout_actor(3, actor)
    assert eng.kernel_name().startswith('s2d_reach_actor_rollout_kernel<'), eng.kernel_name()
    _against_random_policy(eng, cfg, rows, out, 3, name)


def _against_random_policy(eng, cfg, rows, out, T, tag):
    dev = read_out(eng)
    orc = O.OracleEngine(cfg, len(rows), 'f32')
    R.load_rows(orc, rows)
    ref = orc.rollout(T)
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        a, b = out[k].cpu().numpy(), ref[k]
        a, b = (a.view(np.int32), b.view(np.int32)) if a.dtype == f32 else (a, b)
        assert a.shape == b.shape and np.array_equal(a, b), f'{tag}: record {k} differs in {int((a != b).sum())} words'
    last = R.outputs(orc)
    orc.close()
    for i, f in enumerate(R.F):
        a, b = (_bits(dev['state'][:, i]), _bits(last['state'][:, i])) if i < R.NF else (dev['state'][:, i], last['state'][:, i])
        assert np.array_equal(a, b), f'{tag}: state.{f}'
    assert ref['done'].sum() > 20


# ------------------------------------------------------------------------------------------------------------------------ resets
@pytest.mark.parametrize('name', list(R.RESET_CONFIGS))
def test_resets_on_device(name):
    """Engine.reset(), a masked reset at written episode counters and auto-resets reached by writing step_number = max_steps: bitwise
    the fp32 oracle's, and float64's within the reset rule"""
    kw = R.RESET_CONFIGS[name]
    cfg = R.make_cfg(kw)
    n = 2048
    eng = _engine(n, kw)                                     # (_engine resets: the first reset, episode 0 -> 1)
    for ep, mask in ((np.zeros(n, dtype=np.int64), None), R.reset_episodes(n)):
        if mask is not None:
            blank = R.read_rows(O.OracleEngine(cfg, n, 'f32'))
            blank[:, R.IDX['episode']] = ep
            write_rows(eng, blank)
            eng.reset(torch.as_tensor(mask, device='cuda:0'))
            assert eng.kernel_name() == 's2d_reach_reset_kernel'
        dev = read_out(eng)
        orc = R.reset_from(cfg, n, ep, 'f32', mask)
        sel = np.ones(n, bool) if mask is None else mask.astype(bool)
        for i, f in enumerate(R.F):
            a, b = (_bits(dev['state'][:, i]), _bits(orc['state'][:, i])) if i < R.NF else (dev['state'][:, i], orc['state'][:, i])
            assert np.array_equal(a, b), f'{name}: state.{f} after the reset'
        assert np.array_equal(_bits(dev['obs'])[sel], _bits(orc['obs'])[sel]), f'{name}: obs after the reset'
        dev['tries'] = orc['tries']
        rep, fails = R.compare_reset(cfg, n, ep, dev, mask)
        assert not fails, '\n'.join(fails)
        assert rep['skipped'] <= R.TRIES_CAP * rep['n'] and rep['n'] > 900
    # auto-reset inside a step: every env on its last step
    rows = R.read_rows(O.OracleEngine(cfg, n, 'f32'))
    played = R.played_states(cfg, n=n, steps=3, points=1)[0][0]
    rows[:] = played
    rows[:, R.IDX['step_number']] = cfg.task.max_steps
    rows[:, R.IDX['episode']] = R.reset_episodes(n, seed=8)[0]
    a = R.random_actions(np.random.RandomState(2), cfg, n)
    rep, _ = one_cycle(eng, cfg, rows, a, False, _step, f'{name} auto-reset')
    assert rep['ended'] + rep['ill'] == n
