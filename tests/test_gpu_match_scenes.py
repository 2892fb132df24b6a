"""The rule-scene table (tests/match_scenes.py) on the GPU: every scene on the kernel and on the fp32 oracle, from the same initial state
with the same actions -- after every cycle every state word and the stats, and every word of the rollout record, equal bit for bit.
Each scene through the per-step entry point and through s2d_match_rollout_ex (record on), on the instantiation its configuration
selects and, where that is a stock one, on the general one as well.  tests/test_match_scenes_host.py shows what the table reaches."""
import numpy as np
import pytest

import match_oracle as MO
import match_scenes as MS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

STATE_FIELDS = MO.OBJ_FIELDS + ('catch_ban', 'card') + MO.ENV_FIELDS + ('ball_holder', 'goalie_moves', 'set_play_taker', 'last_kicker',
                                                                         'stopped_cycle', 'tick')
CASES = [(sc, g) for sc in MS.SCENES for g in ((False, True) if MS.stock_accepts(sc) else (False,))]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} words differ; first at {i}: gpu={got[i]!r} cpu={want[i]!r}')


def _engine(sc, orc):
    """an engine of the scene's configuration in the oracle's (initial) state"""
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(sc.n, 'cuda:0', cfg=orc.cfg)
    for name, v in orc.snapshot().items():
        getattr(eng, name).copy_(torch.as_tensor(v, device='cuda:0'))
    return eng


def _reset(eng, mask):
    eng.reset(None if mask.all() else torch.as_tensor(mask, device='cuda:0'))


@pytest.mark.parametrize('sc,general', CASES, ids=[f"{sc.name}-{'general' if g else 'own'}" for sc, g in CASES])
def test_scene_on_device(sc, general, monkeypatch):
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    else:
        monkeypatch.delenv('S2D_MATCH_GENERAL_KERNEL', raising=False)
    orc0 = MS.make_oracle(sc)
    step_eng, roll_eng = _engine(sc, orc0), _engine(sc, orc0)
    name = step_eng.kernel_name()
    assert ('<general' in name) == (general or not MS.stock_accepts(sc)), name      # (<general> or <general, illegal defense>)
    for f in STATE_FIELDS:                                                 # the state went in as it is
        _same(getattr(step_eng, f).cpu().numpy(), orc0.get(f), f'{sc.name} initial {f}')
    acts = MS.scene_actions(sc)

    # 1. the per-step entry point, beside the oracle
    def each(t, orc, a, mask):
        if mask is not None:
            _reset(step_eng, mask)
        step_eng.step(None if acts is None else torch.as_tensor(a, device='cuda:0'))
        torch.cuda.synchronize()
        for f in STATE_FIELDS:
            _same(getattr(step_eng, f).cpu().numpy(), orc.get(f), f'{sc.name} [{name}] step t={t} {f}')
        assert list(step_eng.stats.cpu().numpy()) == list(orc.stats()), (sc.name, t)
    tr = MS.run_on_oracle(sc, each=each)
    assert sc.witness(tr), sc.name

    # 2. s2d_match_rollout_ex with the record on: one launch between two resets
    cuts = sorted({0, sc.T} | {t for t, _m in sc.resets})
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        mask = MS.reset_mask(sc, t0)
        if mask is not None:
            _reset(roll_eng, mask)
        a = None if acts is None else torch.as_tensor(acts[t0:t1], device='cuda:0')
        out = roll_eng.rollout(t1 - t0, a, with_obs=True, record_actions=True)
        torch.cuda.synchronize()
        obs = out['obs'].cpu().numpy()
        for k, f in enumerate(('x', 'y', 'vx', 'vy', 'body')):
            _same(obs[:, :, :23, k], tr[f][t0:t1, :, :23], f'{sc.name} [{name}] record obs.{f} cycles {t0}..{t1}')
        _same(out['mode'].cpu().numpy(), tr['mode'][t0:t1], f'{sc.name} record mode')
        _same(out['reward'].cpu().numpy(), tr['reward_left'][t0:t1], f'{sc.name} record reward')
        _same(out['done'].cpu().numpy(), tr['done'][t0:t1], f'{sc.name} record done')
        _same(out['actions'].cpu().numpy(), tr.actions[t0:t1], f'{sc.name} record actions')
        for f in STATE_FIELDS:
            _same(getattr(roll_eng, f).cpu().numpy(), tr[f][t1 - 1], f'{sc.name} [{name}] rollout state after cycle {t1 - 1} {f}')
    assert list(roll_eng.stats.cpu().numpy()) == list(tr['stats'][-1]), sc.name
