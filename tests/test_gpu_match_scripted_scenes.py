"""The in-kernel scripted team (m_scripted_action) on the constructed scenes of tests/scripted_scenes.py: every scene word for word
against the host restatement, against the hand-written answers, and by the float64 rule of tests/scripted_f64.py under
EDGE_ILL_CAP; on the instantiation the configuration selects and on the general one; as one batch and rotated by one match, so that
every scene sits in both halves of a wave.  And the reward gate (chaser_only) names the chaser float64 names."""
import numpy as np
import pytest

import scripted_f64 as F
import scripted_policy as SP
import scripted_scenes as SS
from soccer2d_amd import _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return SP.build(tmp_path_factory.mktemp('scripted_scenes_gpu'))


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('hetero', [False, True])
def test_scene_table_on_the_device(ref, hetero, general, monkeypatch):
    import scripted_device as D
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    cfg = SS.scene_config(hetero)
    prm = SP.params(cfg)
    table = SS.scenes(cfg)
    state, cmd, rule, angles = SS.batch(table)
    n = len(table)
    want = SP.actions(ref, state, prm)
    eng = D.engine(cfg, n)
    assert eng.kernel_name().endswith('controllers>') and ('general' in eng.kernel_name()) == general
    for shift in (0, 1):
        D.load_scene(eng, {k: np.roll(v, shift, axis=0) for k, v in state.items()})
        back = D.read(eng)
        assert all(np.array_equal(back[k], np.roll(state[k], shift, axis=0)) for k in F.KEYS)
        rec = np.roll(D.cycle(eng)[0][0], -shift, axis=0)
        tag = f'{"hetero" if hetero else "default"}, {"general" if general else "selected"}, shift {shift}'
        D.assert_same_words(rec, want, tag)
        fails = SS.check(table, cmd, rule, angles, rec[..., 0], got_ang=F.angle_of(rec))
        assert not fails, '\n'.join([tag] + fails)
        rep, fails = F.compare(state, prm, rec)
        assert not fails, (tag, fails)
        assert rep['share'] <= F.EDGE_ILL_CAP
        fails = SS.check(table, cmd, rule, angles, rec[..., 0], rep['f64']['rule'], F.angle_of(rec), rows=rep['well'])
        assert not fails, '\n'.join([tag] + fails)
    eng.close()


GATE_SCENES = ('a tie of', 'sent off', 'the goalie is the nearest')


def _gate_check(cfg, state, named, held, tag):
    """one cycle with the approach weight alone and chaser_only: within each team in PlayOn a non-zero reward appears only at the
    slot `named` [n, 22] (float64's chaser of the row's team); held [n, 22]: the rows to hold.  Returns (checked, skipped)."""
    import scripted_device as D
    n = len(state['mode'])
    eng = D.engine(cfg, n)
    eng.set_agent_reward({'approach': 1.0}, chaser_only=True)
    D.load_scene(eng, state)
    eng.vx[:, 22], eng.vy[:, 22] = 0.37, -0.23                # the ball moves: every distance changes, whoever is gated
    _, out = D.cycle(eng, agent_reward=True)
    rw = out['agent_reward'][0].cpu().numpy()
    live = ((state['mode'] == M.GM_PLAY_ON) & (out['mode'][0].cpu().numpy() == M.GM_PLAY_ON))[:, None] & held
    is_chaser = named == np.arange(22)[None, :]
    wrong = live & ~is_chaser & (rw != 0.0)
    assert not wrong.any(), (tag, np.argwhere(wrong)[:4], rw[wrong][:4])
    rows = live & is_chaser
    skipped = rows & (rw == 0.0)
    eng.close()
    return int(rows.sum()), int(skipped.sum())


@pytest.mark.parametrize('hetero', [False, True])
def test_reward_gate_names_the_same_chaser(hetero):
    cfg = SS.scene_config(hetero)
    prm = SP.params(cfg)
    table = [sc for sc in SS.scenes(cfg) if any(g in sc.name for g in GATE_SCENES) and int(sc.s['mode'][0]) == M.GM_PLAY_ON]
    assert len(table) >= 12
    state = SS.batch(table)[0]
    # the scenes: exact ties and all, against unprobed float64 (a tie goes to the lowest index there too)
    named = F.decide(state, prm)['search']
    checked, skipped = _gate_check(cfg, state, named, np.ones((len(table), 22), bool), 'scenes')
    # a batch with the ball at somebody's feet: the rows float64 holds under its probes
    state, _ = F.corpus(cfg, 512, 91, strata=(1,))
    state['tackle_cycles'][:] = 0                             # (a tackling chaser does not move; his distance still changes with the ball)
    ref64 = F.decide(state, prm)
    rs = np.random.RandomState(5)
    held = np.ones(ref64['search'].shape, bool)
    for k in range(F.K_PROBES + 2):
        scale = 0 if k < F.K_PROBES else (-1 if k == F.K_PROBES else 1)
        held &= F.decide(F.OF.perturb(state, rs, scale=scale), prm)['search'] == ref64['search']
    assert held.mean() >= 1.0 - F.ILL_CAP
    c2, s2 = _gate_check(cfg, state, ref64['search'], held, 'ball at a player')
    print(f'reward gate: {checked + c2} chaser rows checked, {skipped + s2} skipped with an approach term of exactly 0')
    assert checked + c2 >= 400 and skipped + s2 <= 0.05 * (checked + c2)
