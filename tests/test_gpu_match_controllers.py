"""11v11 engine with per-slot controllers on the GPU: the in-kernel scripted team chooses what the host restatement
(tests/scripted_policy_ref.c) chooses, bit for bit; its recorded actions drive the CPU oracle to the same states; mixed
tables read only the caller's rows and keep the random policy's draws; the scripted team beats the random one."""
import numpy as np
import pytest

import match_oracle as MO
import scripted_policy as SP
from test_gpu_match import _pair, assert_match_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return SP.build(tmp_path_factory.mktemp('scripted'))


def _state(eng):
    return {k: getattr(eng, k).cpu().numpy() for k in SP.OBJ_PLANES + SP.ENV_WORDS}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_actions_equal(got, want, tag):
    if not np.array_equal(_bits(got), _bits(want)):
        bad = np.argwhere(_bits(got) != _bits(want))
        e, p, w = bad[0]
        raise AssertionError(f'{tag}: {len(bad)} words differ; first match {e} player {p} word {w}: gpu={got[e, p]} host={want[e, p]}')


@pytest.mark.parametrize('general', [False, True])
def test_scripted_policy_is_the_rule_table_and_drives_the_oracle(ref, general, monkeypatch):
    """Both teams scripted, one cycle per launch: every recorded (cmd, a, b) equals the host restatement applied to the state
    read before the cycle, and the recorded actions fed to the oracle give the same state after every cycle.  Noise is on, so
    that the matches (all started from the same kick-off by a deterministic policy) play different games; it leaves the stock
    rules in their instantiation."""
    n, T = (4096, 300) if not general else (1024, 300)
    kw = dict(noise=True, seed=11 if general else 0x5EED)
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    eng, orc = _pair(n, **kw)
    eng.set_controllers({'left': 'scripted', 'right': 'scripted'})
    assert eng.kernel_name().endswith('controllers>') and ('general' in eng.kernel_name()) == general
    prm = SP.params(eng.cfg)
    eng.reset(); orc.reset()
    out = eng.alloc_rollout(1, with_obs=False, record_actions=True)
    seen, cmds = set(), set()
    for t in range(T):
        s = _state(eng)
        seen.update(np.unique(s['mode']).tolist())
        eng.rollout(1, out=out, record_actions=True)
        rec = out['actions'][0].cpu().numpy()
        _assert_actions_equal(rec, SP.actions(ref, s, prm), f'cycle {t}')
        cmds.update(np.unique(rec[:, :, 0]).tolist())
        orc.step(rec)
        assert_match_same(eng, orc, f'cycle {t}')
    assert len(seen) >= 4, seen                            # kick-off, play on and restarts were played
    assert {0.0, 1.0, 2.0, 3.0} <= cmds, cmds
    assert len(np.unique(eng.x.cpu().numpy()[:, 22])) > n // 4   # the matches differ


def test_scripted_fused_rollout_drives_the_oracle():
    """T = 64 in one launch: the record, fed to the oracle cycle by cycle, reproduces every recorded observation and the end state."""
    n, T = 2048, 64
    eng, orc = _pair(n, noise=True)
    eng.set_controllers([2] * 22)
    eng.reset(); orc.reset()
    for _ in range(3):
        out = eng.rollout(T, record_actions=True)
        rec = out['actions'].cpu().numpy()
        obs = out['obs'].cpu().numpy()
        for t in range(T):
            orc.step(rec[t])
            want = np.stack([orc.get(f) for f in ('x', 'y', 'vx', 'vy', 'body')], axis=2)
            assert np.array_equal(_bits(obs[t]), _bits(want)), t
        assert_match_same(eng, orc, 'end of launch')


def test_external_rows_of_other_slots_are_never_read():
    """Left external, right scripted: NaN in the right team's caller rows changes nothing, and the oracle fed the merged
    actions (caller's left rows + recorded right rows) gives the same states."""
    n, T = 2048, 64
    g = torch.Generator(device='cuda:0').manual_seed(7)
    cmd = torch.randint(1, 5, (T, n, 22, 1), device='cuda:0', generator=g).float()
    mag = torch.rand((T, n, 22, 2), device='cuda:0', generator=g) * 200.0 - 100.0
    acts = torch.cat([cmd, mag], dim=3)
    nan_acts = acts.clone()
    nan_acts[:, :, 11:] = float('nan')
    runs = []
    for a in (acts, nan_acts):
        eng, orc = _pair(n)
        eng.set_controllers({'left': 'external', 'right': 'scripted'})
        eng.reset()
        out = eng.rollout(T, actions=a, record_actions=True)
        runs.append((eng, orc, {k: v.cpu().numpy() for k, v in out.items() if v is not None}))
    (e0, o0, r0), (e1, _, r1) = runs
    for k in r0:
        assert np.array_equal(_bits(r0[k]), _bits(r1[k])), k
    rec = r0['actions']
    assert np.array_equal(_bits(rec[:, :, :11]), _bits(acts[:, :, :11].cpu().numpy()))
    o0.reset()
    for t in range(T):
        o0.step(rec[t])
    assert_match_same(e0, o0, 'external left + scripted right')
    assert_match_same(e1, o0, 'NaN rows')


def test_random_slots_draw_what_the_table_less_engine_draws():
    n, T = 2048, 64
    mixed, _ = _pair(n)
    plain, _ = _pair(n)
    mixed.set_controllers({'left': 'random', 'right': 'scripted'})
    mixed.reset(); plain.reset()
    for _ in range(2):
        a = mixed.rollout(T, record_actions=True)['actions'].cpu().numpy()
        b = plain.rollout(T, record_actions=True)['actions'].cpu().numpy()     # no table, actions None: the random policy
        assert np.array_equal(_bits(a[:, :, :11]), _bits(b[:, :, :11]))
        assert not np.array_equal(_bits(a[:, :, 11:]), _bits(b[:, :, 11:]))
    # the record of a table-less launch is the draw the engine itself replays: the oracle's random policy
    plain2, orc = _pair(n)
    plain2.reset(); orc.reset()
    out = plain2.rollout(1, record_actions=True)
    assert np.array_equal(_bits(out['actions'][0].cpu().numpy()), _bits(orc.random_actions()))
    # back to no table: the launch is today's kernel again
    mixed.set_controllers(None)
    assert not mixed.kernel_name().endswith('controllers>')


def test_controller_errors_on_device():
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(64, 'cuda:0')
    import ctypes as C
    lib = eng.lib
    bad = (C.c_uint8 * 22)(*([0] * 21 + [3]))
    assert lib.s2d_match_set_controllers(eng._h, bad) != 0 and b'slot 21' in lib.s2d_last_error()
    eng.set_controllers({'left': 'external', 'right': 'scripted'})
    with pytest.raises(ValueError, match='external'):
        eng.rollout(4)                           # an external slot and no actions
    with pytest.raises(ValueError, match='external'):
        eng.step(None)
    raw = torch.empty(4 * 64 * 22 * 3 + 1, dtype=torch.float32, device='cuda:0')
    rc = lib.s2d_match_rollout_ex(eng._h, 1, None, None, C.c_void_p(raw.data_ptr() + 2), None)
    assert rc != 0 and b'aligned' in lib.s2d_last_error()


def test_vec_env_against_in_kernel_opponent():
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    env = Soccer2DMatchVecEnv(256, opponent='scripted')
    assert env.action_space.shape == (11, 3)
    obs = env.reset()
    ref = Soccer2DMatchVecEnv(256)
    ref.reset()
    ref.engine.set_controllers({'left': 'external', 'right': 'scripted'})
    a = torch.zeros((256, 11, 3), device='cuda:0')
    a[:, :, 0] = 1.0
    a[:, :, 1] = 50.0
    full = torch.zeros((256, 22, 3), device='cuda:0')
    full[:, :11] = a
    for _ in range(20):
        obs, rew, done, info = env.step(a)
        obs2, _, _, _ = ref.step(full)
        assert torch.equal(obs, obs2)
    assert obs.shape == (256, 23, 5)
    with pytest.raises(ValueError):
        env.step(torch.zeros((256, 22, 3), device='cuda:0'))


def test_scripted_team_beats_random():
    """2 048 matches of 2 x 300 cycles, scripted left vs random right.  The threshold was set from the first correct run, which
    ended 6 608 : 0 (profiles/r05/match_controllers.txt), with a wide margin: more than 3 x the random team's goals and at least
    one goal per match on average."""
    from soccer2d_amd.match import MatchEngine
    n = 2048
    eng = MatchEngine(n, 'cuda:0', half_time_cycles=300, nr_extra_halfs=0, penalty_shoot_outs=0, auto_reset=False)
    eng.set_controllers({'left': 'scripted', 'right': 'random'})
    eng.reset()
    for _ in range(40):                                  # far past the end: stopped cycles, extra time and the shoot-out included
        eng.rollout(64, with_obs=False)
        if bool((eng.mode == MO.M.GM_TIME_OVER).all()):
            break
    assert bool((eng.mode == MO.M.GM_TIME_OVER).all())
    gl, gr = int(eng.score_left.sum()), int(eng.score_right.sum())
    print(f'scripted vs random: goals {gl} : {gr} in {n} matches')
    assert gl > 3 * gr and gl >= n, (gl, gr)
