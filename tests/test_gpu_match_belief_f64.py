"""The belief kernel (s2d_match_belief_scan) against the float64 update written from the header's five steps (tests/belief_f64.py),
by that module's rule: on random rows (random prior beliefs over random well-formed see rows, two parameter sets) and on a record
played by the engine, every update taken one at a time from the fp32 state before it.  The same outputs equal the host
restatement (tests/belief_ref.c) bit for bit, so the device needs no margin beyond the restatement's
(tests/test_belief_f64_host.py carries the measured figures); the cap on ill-conditioned rows is ILL_CAP itself."""
import ctypes as C

import numpy as np
import pytest

import belief as B
import belief_f64 as F
from soccer2d_amd import _capi, _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
OTHER = dict(ball_decay=0.9, player_decay=0.5, view_angle=(50.0, 100.0, 170.0), match_dist=2.0, match_rate=0.05, ghost_margin=3.0,
             count_max=6.0)
SHORT = dict(noise=True, half_time_cycles=10, nr_extra_halfs=0, penalty_shoot_outs=0, after_goal_wait=5)


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return B.build(tmp_path_factory.mktemp('belief_ref'))


def _same(got, want, tag):
    g, w = np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f'{tag}: {len(bad)} words differ; first at {tuple(bad[0])}: gpu={got[tuple(bad[0])]!r} '
                             f'host={want[tuple(bad[0])]!r}')


def _report(tag, rep):
    print(f"{tag}: {rep['n']} rows, {rep['ill']} ill-conditioned ({100 * rep['share']:.3f} %); " +
          ', '.join(f"{k} {rep['worst'][k]:.2f} raw {rep['raw'][k]:.2f} (T {F.T_ULPS[k]:.2f})" for k in ('pos', 'vel', 'body')))


@pytest.mark.parametrize('tag, over', [('default', {}), ('other', OTHER)])
def test_random_rows(ref, tag, over):
    """300 matches x 22 agents, one update: agent row r of every match is the agent of slot r"""
    lib = M.bind(_capi.load_library())
    n, P = 300, F.values(**over)
    bel, see, flag, _slot = F.random_rows(np.random.default_rng(40 + len(over)), n * 22, P)
    assert F.in_domain(bel, see, P)
    flag = flag[:n]
    s, b = torch.from_numpy(see).cuda(), torch.from_numpy(bel).cuda()
    r = torch.from_numpy(flag).cuda()
    prm = M.belief_params(lib, **over)
    _capi.check(lib, lib.s2d_match_belief_scan(C.byref(prm), s.data_ptr(), r.data_ptr(), b.data_ptr(), None, 1, n, 0x3FFFFF, None),
                's2d_match_belief_scan')
    torch.cuda.synchronize()
    got = b.cpu().numpy()
    _same(got, B.step(ref, B.params(**over), see.reshape(n, 22, 192), bel.reshape(n, 22, 192), flag).reshape(-1, 192), 'restatement')
    rep, fails = F.compare(got, bel, see, np.repeat(flag, 22), np.tile(np.arange(22) % 11, n), P)
    _report(f'random, {tag}', rep)
    a = rep['disc']['assign']
    assert (a >= 0).sum() > 5000 and (a == -1).sum() > 5000 and rep['disc']['ghost'].sum() > 1000
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP, rep['share']


def test_played_record(ref):
    """40 cycles of 12 matches, scripted against scripted, random view actions, matches restarting: each belief_step against
    float64 from the device's own state before it"""
    from soccer2d_amd.match import MatchEngine
    n, T = 12, 40
    eng = MatchEngine(n, 'cuda:0', seed=11, **SHORT)
    eng.set_controllers({'left': 'scripted', 'right': 'scripted'})
    eng.enable_vision()
    eng.enable_belief('all')
    eng.reset()
    g = torch.Generator(device='cuda:0').manual_seed(3)
    rows = []
    for _ in range(T):
        eng.step(None)
        v = torch.empty((n, 22, 2), device='cuda:0')
        v[..., 0] = torch.rand((n, 22), device='cuda:0', generator=g) * 180 - 90
        v[..., 1] = torch.randint(0, 4, (n, 22), device='cuda:0', generator=g).float() * (torch.rand((n, 22), device='cuda:0', generator=g) < 0.3)
        eng.vision_step(v, done=True)
        see, before, done = eng.see('all'), eng.belief.clone(), eng.done.clone()
        after = eng.belief_step(see, done=True)
        rows.append([x.cpu().numpy() for x in (before, see, done, after)])
    eng.close()
    bel, see, after = (np.concatenate([r[i].reshape(-1, 192) for r in rows]) for i in (0, 1, 3))
    flag = np.concatenate([np.repeat(r[2].astype(np.uint8), 22) for r in rows])
    slot = np.tile(np.arange(22), n * T)
    P = F.values()
    assert F.in_domain(bel, see, P) and flag.any()
    _same(after, F.restatement(ref, {}, bel, see, flag, slot), 'restatement')
    rep, fails = F.compare(after, bel, see, flag, slot % 11, P)
    _report('played', rep)
    a = rep['disc']['assign']
    assert (a >= 0).sum() > 500 and (a == -1).sum() > 100 and rep['disc']['ghost'].sum() > 100
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP, rep['share']
