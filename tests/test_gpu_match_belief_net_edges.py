"""belief_update() of csrc/s2d_belief_row.h -- the copy of the belief rule that the BELIEF instantiations of the cycle kernel run --
at the rule's edges and against float64.  tests/test_gpu_match_belief_net.py holds it to the scan kernel on played rows; here:

  a. the state scenes of tests/belief_state_scenes.py, one match per scene and T = 1: the recorded see row is see_ref's and holds
     what the scene states, the recorded belief row is the hand-written answer, belief_ref's and belief_scan's on a twin, bit for
     bit; both kernels, and two orders of the table so that every scene runs in either half of a wave beside a scene that takes
     other branches (the gate, the pending loop, the reset flag), once with an empty half in the last wave; one scene at n = 1;
  b. T = 3 over the counts and gate scenes: count_max - 2 -> count_max - 1 -> forgotten inside one launch;
  c. a played record of 33 cycles, every update against float64 by the rule of tests/belief_f64.py (T_ULPS and ILL_CAP as they
     are) and against belief_ref bit for bit;
  d. random in-domain priors written over the belief after 0, 5 and 17 cycles of play, one cycle: matched, unmatched and ghost
     updates that play from an unknown belief does not reach; two parameter sets.

The floors of c and d and the ill-conditioned shares were chosen on the CPU from the reference alone (the same seeds replayed
through oracle -> see_ref -> belief_ref -> see_policy_ref: tests/test_belief_state_scenes_host.py, test_reference_replay_figures,
whose docstring keeps the figures)."""
import numpy as np
import pytest

import belief as B
import belief_f64 as F
import belief_scenes as SC
import belief_state_scenes as SS
import match_see as S
from test_gpu_match_belief_f64 import OTHER, SHORT
from test_gpu_match_belief_net import ALL, SCRIPTED, _i32, _policy, _table
from test_gpu_match_f64 import KERNELS
from test_gpu_match_see import _state, _write
from test_gpu_match_see_net import _same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
REC = dict(with_obs=False, net_index=True, logp=True, see_obs='all', belief_obs='all')
# c and d: the seeds and sizes the host replay uses too
PLAYED = dict(n=12, T=33, seed=11, net=(16, 16, 16, 3))
PRIORS = dict(n=48, cycles=(0, 5, 17), seed=17, net=(16, 16, 16, 3), floors={'default': (800, 3300, 1800), 'other': (280, 3900, 1700)})


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('belief_net_edges')
    return dict(see=S.build(d), bel=B.build(d))


def _engine(n, actor=None, bover=None, vision=None, seed=5, **kw):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(n, 'cuda:0', seed=seed, **kw)
    eng.set_controllers(SCRIPTED)
    eng.enable_vision(**(vision or {}))
    eng.enable_belief('all', **(bover or {}))
    if actor is not None:
        eng.set_network(actor, ALL)
    eng.reset()
    return eng


def _still_actor():
    """the small tanh policy, with a table that neither turns a neck nor changes a view: the see timer runs undisturbed"""
    actor = _policy(16, 16, 16, 'tanh', seed=3)
    tab = _table(16, 3)
    tab[:, 3:5] = 0.0
    actor.set_table(tab)
    return actor


def _kernel(eng, general):
    name = eng.kernel_name()
    assert name.endswith(', belief network>') and ('general' in name) == general, name
    if not general:
        assert name == f's2d_match_rollout_kernel<{KERNELS[0][0]}, belief network>', name


def _launch_scenes(refs, scenes, prm, shift, T, general, actor):
    """scenes of one parameter set, scene i in match i + shift (the matches before: as reset() leaves them); one launch of T
    cycles.  Returns what the comparisons need."""
    n = len(scenes) + shift
    over = SS.belief_over(prm)
    eng = _engine(n, actor, over, SS.VISION, **KERNELS[0][1])
    twin = _engine(n, None, over, SS.VISION, **KERNELS[0][1])
    _kernel(eng, general)
    st = _state(eng)
    flags = np.zeros(n, dtype=np.uint8)
    bel0 = eng.belief.cpu().numpy()
    for i, s in enumerate(scenes):
        flags[i + shift] = SS.write_state(st, i + shift, s)
        bel0[i + shift, s.slot] = s.prior
    _write(eng, st)
    eng.done.copy_(torch.from_numpy(flags))
    eng.belief.copy_(torch.from_numpy(bel0))
    twin.belief.copy_(eng.belief)
    want_see = S.see(refs['see'], st, S.params(seed=eng.cfg.seed, env_id_offset=eng.cfg.env_id_offset, **SS.VISION))
    out = eng.rollout(T, **REC)
    torch.cuda.synchronize()
    see, bel, done = (out[k].cpu().numpy() for k in ('see', 'belief', 'done'))
    assert see.shape == bel.shape == (T, n, 22, 192)
    _same(see[0], want_see, f'[{prm}] the first see rows against see_ref')
    fl = np.concatenate([flags[None], done[:T - 1]])
    got = twin.belief_scan(out['see'], reset=torch.from_numpy(fl).cuda(), out=True)
    assert torch.equal(_i32(out['belief']), _i32(got)), f'[{prm}] record against belief_scan'
    assert torch.equal(_i32(eng.belief), _i32(out['belief'][T - 1])), f'[{prm}] the state is the last row of the record'
    _, hrec = B.scan(refs['bel'], B.params(**SS.PARAMS[prm]), see, bel0, fl)
    _same(bel, hrec, f'[{prm}] record against belief_ref')
    eng.close(); twin.close()
    return see, bel, hrec, fl


def _check_answers(scenes, see, bel, shift, prm):
    wrong = []
    for i, s in enumerate(scenes):
        row, got = see[0, i + shift, s.slot], bel[0, i + shift, s.slot]
        wrong += [f'{s.name} [{prm}]: the see row: {b}' for b in s.check_see(row)]
        want = s.answer(row)
        d = SC.same_row(got, want)
        if len(d):
            wrong.append(f'{s.name} [{prm}] (match {i + shift}): word {d[0]}: {got[d[0]]!r}, the answer is {want[d[0]]!r} ({len(d)} words differ)')
    return wrong


# ------------------------------------------------------------------------------------------ a. the table
@pytest.mark.parametrize('shift', [0, 1], ids=['as ordered', 'shifted by one match'])
@pytest.mark.parametrize('general', [False, True], ids=['stock', 'general'])
def test_the_table_through_the_cycle_kernel(refs, general, shift, monkeypatch):
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    T = SS.table()
    actor = _policy(16, 16, 16, 'tanh', seed=3)
    wrong, seen, sizes = [], set(), []
    for prm in SS.USED:
        scenes = SS.launch_order([s for s in T if s.prm == prm])
        seen |= SS.divergences([None] * shift + [SS.kind(s) for s in scenes])
        sizes.append(len(scenes) + shift)
        see, bel, _, _ = _launch_scenes(refs, scenes, prm, shift, 1, general, actor)
        wrong += _check_answers(scenes, see, bel, shift, prm)
    assert not wrong, '\n'.join(wrong)
    # from the table, not from the device: the two halves of some wave diverged at the gate, at the pending loop, at the reset flag
    assert seen == {'can', 'pending', 'reset'}, seen
    assert any(k % 2 for k in sizes), sizes                # a last wave with an empty half


@pytest.mark.parametrize('general', [False, True], ids=['stock', 'general'])
def test_one_scene_alone(refs, general, monkeypatch):
    """n = 1: one half-wave in the launch"""
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    actor = _policy(16, 16, 16, 'tanh', seed=3)
    wrong = []
    for name in ('tie of three, rows 2, 6 and 9', 'done byte 255 before the launch', 'a level-4 row names the entry an earlier level-3 row is nearest to'):
        scenes = [s for s in SS.table() if s.name == name]
        assert len(scenes) == 1
        see, bel, _, _ = _launch_scenes(refs, scenes, scenes[0].prm, 0, 1, general, actor)
        wrong += _check_answers(scenes, see, bel, 0, scenes[0].prm)
    assert not wrong, '\n'.join(wrong)


# ------------------------------------------------------------------------------------------ b. ageing inside one launch
@pytest.mark.parametrize('prm', ['default', 'cm1', 'cm2', 'other'])
def test_ageing_across_the_cycles_of_one_launch(refs, prm):
    """T = 3 on the counts and gate scenes; nobody turns a neck or changes a view, so an agent that was fresh in the first cycle is
    not in the next two and its entries only age: count_max - 2 -> count_max - 1 -> forgotten inside one launch"""
    scenes = SS.launch_order([s for s in SS.table() if s.prm == prm and s.bullet in ('counts', 'gate')])
    assert scenes
    T, cm = 3, SC.count_max(prm)
    see, bel, hrec, fl = _launch_scenes(refs, scenes, prm, 0, T, False, _still_actor())
    assert not _check_answers(scenes, see, bel, 0, prm)
    assert not fl[1:].any()                                # (no match ended: nothing was reset on the way)
    aged = 0
    for i, s in enumerate(scenes):
        if s.can and s.width == 3:                         # (a sent-off agent's see timer stands still)
            assert (see[1:, i, s.slot, 8] == 0).all(), s.name
            pc = hrec[:, i, s.slot, 29::8]                 # [T, 21], the reference's
            aged += int(((pc[0] == cm - 2) & (pc[1] == cm - 1) & (pc[2] == cm)).sum()) if cm >= 3 else int(((pc[0] < cm) & (pc[T - 1] == cm)).sum())
    if prm != 'default':                                   # (the gate scenes' entries are young)
        assert aged > 0 or cm == 1, (prm, aged)


# ------------------------------------------------------------------------------------------ c. the record against float64
def _report(tag, rep):
    print(f"{tag}: {rep['n']} rows, {rep['ill']} ill-conditioned ({100 * rep['share']:.3f} %); " +
          ', '.join(f"{k} {rep['worst'][k]:.2f} raw {rep['raw'][k]:.2f} (T {F.T_ULPS[k]:.2f})" for k in ('pos', 'vel', 'body')))


def test_played_record_against_float64(refs):
    """12 matches x 33 cycles in ONE launch, all 22 slots on a policy whose table turns necks both ways and changes views, halves
    of 10 cycles: recorded row t is one update of (row t - 1, or the state before the launch; see row t; flag t)"""
    n, T = PLAYED['n'], PLAYED['T']
    h1, h2, k, seed = PLAYED['net']
    actor = _policy(h1, h2, k, 'tanh', seed=seed)
    tab = actor.table.cpu().numpy()
    assert set(tab[:, 4].tolist()) == {0.0, 1.0, 2.0, 3.0} and (tab[:, 3] > 0).any() and (tab[:, 3] < 0).any()
    eng = _engine(n, actor, seed=PLAYED['seed'], **SHORT)
    before, done0 = eng.belief.cpu().numpy(), eng.done.cpu().numpy()
    out = eng.rollout(T, **REC)
    torch.cuda.synchronize()
    see, bel, done = (out[k].cpu().numpy() for k in ('see', 'belief', 'done'))
    eng.close()
    prev = np.concatenate([before[None], bel[:-1]]).reshape(-1, 192)
    flag = np.repeat(np.concatenate([done0[None], done[:-1]]).reshape(-1), 22)
    slot = np.tile(np.arange(22), n * T)
    see, after = see.reshape(-1, 192), bel.reshape(-1, 192)
    P = F.values()
    assert F.in_domain(prev, see, P) and flag.any()
    _same(after, F.restatement(refs['bel'], {}, prev, see, flag, slot), 'restatement')
    rep, fails = F.compare(after, prev, see, flag, slot % 11, P)
    _report('cycle kernel, played', rep)
    a = rep['disc']['assign']
    print(f"assigned {(a >= 0).sum()}, unassigned {(a == -1).sum()}, ghosts {rep['disc']['ghost'].sum()}, flags {flag.sum() // 22}")
    assert (a >= 0).sum() > 500 and (a == -1).sum() > 100 and rep['disc']['ghost'].sum() > 100
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP, rep['share']


# ------------------------------------------------------------------------------------------ d. random priors over played rows
@pytest.mark.parametrize('tag, over', [('default', {}), ('other', OTHER)])
def test_random_priors_over_played_see_rows(refs, tag, over):
    n = PRIORS['n']
    h1, h2, k, seed = PRIORS['net']
    actor = _policy(h1, h2, k, 'tanh', seed=seed)
    eng = _engine(n, actor, over, seed=PRIORS['seed'], **SHORT)
    P = F.values(**over)
    rng = np.random.default_rng(50 + len(over))
    rows, played = [], 0
    for cycles in PRIORS['cycles']:
        if cycles > played:
            eng.rollout(cycles - played, with_obs=False, belief_obs='all')
            played = cycles
        prior = F.random_rows(rng, n * 22, P)[0].reshape(n, 22, 192)
        eng.belief.copy_(torch.from_numpy(prior))
        done0 = eng.done.cpu().numpy()
        out = eng.rollout(1, **REC)
        played += 1
        torch.cuda.synchronize()
        assert torch.equal(_i32(eng.belief), _i32(out['belief'][0]))
        rows.append((prior, out['see'][0].cpu().numpy(), np.repeat(done0, 22), out['belief'][0].cpu().numpy()))
    eng.close()
    prior, see, after = (np.concatenate([r[i].reshape(-1, 192) for r in rows]) for i in (0, 1, 3))
    flag = np.concatenate([r[2] for r in rows])
    slot = np.tile(np.arange(22), n * len(rows))
    assert F.in_domain(prior, see, P)
    _same(after, F.restatement(refs['bel'], over, prior, see, flag, slot), 'restatement')
    rep, fails = F.compare(after, prior, see, flag, slot % 11, P)
    _report(f'cycle kernel, random priors, {tag}', rep)
    a = rep['disc']['assign']
    print(f"assigned {(a >= 0).sum()}, unassigned {(a == -1).sum()}, ghosts {rep['disc']['ghost'].sum()}")
    lo = PRIORS['floors'][tag]
    assert (a >= 0).sum() > lo[0] and (a == -1).sum() > lo[1] and rep['disc']['ghost'].sum() > lo[2], lo
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP, rep['share']
