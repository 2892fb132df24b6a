"""CPU: the host restatement of the belief layer (tests/belief_ref.c) against the float64 update written from the header's five steps
(tests/belief_f64.py), by that module's rule, and the constructed scenes with hand-written answers (tests/belief_scenes.py).  The
device is held to the same rule and the same scenes in tests/test_gpu_match_belief_f64.py and tests/test_gpu_match_belief_edges.py;
it must equal the restatement bit for bit, so it gets no margin of its own.

Three inputs: random rows (random prior beliefs over random well-formed see rows, two parameter sets); rows played by the host
closed loop of match oracle, see restatement and belief restatement (every update taken one at a time from the fp32 state before
it, never accumulated in float64); every scene of the table.  The restatement may have at most HALF the cap of ill-conditioned
rows (the device test asserts the cap itself).

Measured here (this file's output; the bound T is derived in tests/belief_f64.py, not fitted): the figure held against T is
max over well-conditioned rows of (|f32 - f64| - 2 spread) / UNIT; `raw` is max |f32 - f64| / UNIT.

    input                rows   ill-conditioned   pos (T 18.32)    vel (T 44.65)    body (T 1.00)
    random, default      6000    0  (0.000 %)     1.54  raw 6.91   0.24  raw 4.02   1.00  raw 1.00
    random, other        6000    0  (0.000 %)     0.65  raw 7.34   0.45  raw 4.41   0.50  raw 1.00
    played, 60 cycles    5280    0  (0.000 %)     0.04  raw 1.60   0.02  raw 1.20   0.00  raw 1.00
    scenes                242   15  (6.198 %)     0.00  raw 0.00   0.00  raw 0.00   0.00  raw 0.00

The cycle kernel's copy of the rule (belief_update() in csrc/s2d_belief_row.h), on the records of its own launches
(tests/test_gpu_match_belief_net_edges.py; the same launches replayed on the host in tests/test_belief_state_scenes_host.py give
these rows bit for bit):

    cycle kernel, played 12 x 33     8712    0  (0.000 %)     0.34  raw 1.59   0.00  raw 1.49   0.00  raw 1.00
    cycle kernel, priors, default    3168    1  (0.032 %)     0.31  raw 1.46   0.00  raw 1.28   0.00  raw 1.00
    cycle kernel, priors, other      3168    0  (0.000 %)     0.23  raw 1.41   0.00  raw 1.01   0.00  raw 1.00
    state scenes                      189   13  (6.878 %)     0.00  raw 0.00   0.00  raw 0.00   0.00  raw 0.00

(body reaches its bound: body_rel + face is a tie in [256, 512) whenever face has an odd last bit in [128, 256), and where two probe
moves cancel the spread is 0.  The errors are whole multiples of 2^-16 there, so the comparison with T = 1 is exact.)
(The scenes are exact: every deviation is 0, so nothing exceeds twice the spread.)"""
import numpy as np
import pytest

import belief as B
import belief_f64 as F
import belief_scenes as SC

f32 = np.float32
OTHER = dict(ball_decay=0.9, player_decay=0.5, view_angle=(50.0, 100.0, 170.0), match_dist=2.0, match_rate=0.05, ghost_margin=3.0,
             count_max=6.0)                               # tests/test_gpu_match_belief.py's


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return B.build(tmp_path_factory.mktemp('belief_ref'))


def line(tag, rep):
    w, r = rep['worst'], rep['raw']
    return (f"{tag:<24} {rep['n']:>6}   {rep['ill']:<6} ({100 * rep['share']:.3f} %)   " +
            '   '.join(f"{w[k]:.2f}  raw {r[k]:.2f} (T {F.T_ULPS[k]:.2f})" for k in ('pos', 'vel', 'body')))


def test_derived_bounds():
    """the table is the derivation beside it, evaluated: nothing fitted"""
    assert 18.0 < F.T_ULPS['pos'] < 18.7 and 44.0 < F.T_ULPS['vel'] < 45.3 and F.T_ULPS['body'] == 1.0
    assert (F.K_PROBES, F.PROBE_ULPS, F.ILL_CAP, F.EDGE_ILL_CAP) == (4, 3, 0.01, 0.15)


@pytest.mark.parametrize('tag, over', [('default', {}), ('other', OTHER)])
def test_random_rows(ref, tag, over):
    P = F.values(**over)
    bel, see, flag, slot = F.random_rows(np.random.default_rng(20 + len(over)), 6000, P)
    assert F.in_domain(bel, see, P)
    got = F.restatement(ref, over, bel, see, flag, slot)
    rep, fails = F.compare(got, bel, see, flag, slot % 11, P)
    print(line(f'random, {tag}', rep))
    a, cm = rep['disc']['assign'], P['count_max']
    known = F.unpack(rep['f64'])[..., F.PC] < cm
    # every step of the update takes part, in both outcomes
    assert (a >= 0).sum() > 5000 and (a == -1).sum() > 5000 and rep['disc']['ghost'].sum() > 1000 and 0.3 < known.mean() < 0.8
    assert flag.sum() > 100 and (see[:, 8] == 0).sum() > 100 and (see[:, 15] == 2).sum() > 100
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP / 2, rep['share']


def played_rows(ref, tmp_path_factory, n=4, T=60):
    """tests/test_belief_host.py's closed loop (match oracle -> see restatement -> belief restatement), kept as single updates:
    (belief before, see row, flag, slot, belief after) of every agent and cycle"""
    import match_oracle as MO
    import match_see as S
    import scripted_policy as SP
    cfg = MO.make_match_config(seed=21, noise=1, half_time_cycles=25, nr_extra_halfs=0, penalty_shoot_outs=0)
    orc = MO.MatchOracle(cfg, n)
    orc.reset()
    see_lib, sp_lib = S.build(tmp_path_factory.mktemp('see_ref')), SP.build(tmp_path_factory.mktemp('scripted'))
    sprm, vprm, bprm = SP.params(cfg), S.params(seed=cfg.seed, env_id_offset=cfg.env_id_offset), B.params()
    rng = np.random.default_rng(8)
    planes = {'neck': np.zeros((n, 24), dtype=f32), 'view_width': np.full((n, 24), 2, dtype=np.int32),
              'see_wait': np.zeros((n, 24), dtype=np.int32)}
    bel = B.reset(ref, np.zeros((n, 22, 192), dtype=f32))
    rows = []
    for _ in range(T):
        orc.step(SP.actions(sp_lib, orc.snapshot(), sprm))
        st = orc.snapshot()
        done = st['done']
        v = np.zeros((n, 22, 2), dtype=f32)
        v[..., 0] = rng.uniform(-90, 90, (n, 22))
        v[..., 1] = rng.integers(0, 4, (n, 22)) * (rng.random((n, 22)) < 0.3)
        planes = S.vision_step(see_lib, dict(st, **planes), vprm, v, done)
        see = S.see(see_lib, dict(st, **planes), vprm)
        after = B.step(ref, bprm, see, bel, done)
        rows.append((bel, see, np.repeat(np.asarray(done, dtype=np.uint8)[:, None], 22, axis=1), np.tile(np.arange(22), (n, 1)), after))
        bel = after
    return [np.concatenate([r[i].reshape((-1,) + r[i].shape[2:]) for r in rows]) for i in range(5)]


def test_played_rows(ref, tmp_path_factory):
    bel, see, flag, slot, got = played_rows(ref, tmp_path_factory)
    P = F.values()
    assert F.in_domain(bel, see, P)
    rep, fails = F.compare(got, bel, see, flag, slot % 11, P)
    print(line('played, 60 cycles', rep))
    a = rep['disc']['assign']
    assert (a >= 0).sum() > 500 and (a == -1).sum() > 100 and rep['disc']['ghost'].sum() > 100 and flag.sum() > 0
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP / 2, rep['share']


def test_scenes_cover_every_bullet():
    """so that a later edit cannot quietly drop a scene the table is there for"""
    T = SC.table()
    assert {s.bullet for s in T} == set(SC.BULLETS) and len({s.name for s in T}) == len(T)
    names = ' | '.join(s.name for s in T)
    for r in range(21):
        assert f'level 2: nearest in row {r}' in names
    for a, b in ((0, 1), (3, 4), (14, 15), (15, 16), (9, 10)):
        assert f'tie between rows {a} and {b}' in names
    for slot in range(22):
        assert f'all 21 identities seen from slot {slot} (default)' in names and f'junk identities seen from slot {slot} (default)' in names
    for word in ('> 0', '< 0', '+0', '-0', 'NaN'):
        assert f'team word {word}, row 9 nearer' in names and f'team word {word}, row 10 nearer' in names
    for tag in ('q == tol^2 exactly', 'next float above tol', 'match_dist = 0', 'match_rate = 0', 'dist = +inf', 'dist = NaN', 'fresh = 0',
                'fresh = 2', 'card = red', 'level 0 ', 'level 0.5', 'level 5', 'level -1', 'level NaN', 'ball level 1', 'ball level 2',
                'ball level 3', 'ball level 4', 'level 4 with dist = 0', '(d = 0) is kept', 'exactly on the cone', 'next float outside the cone',
                'behind at +180', 'behind at -180', 'view code 1', 'view code 2', 'view code 3', 'view code 0', 'view code 7', 'view code NaN',
                'negative cone', 'ball as a ghost', 'count_max 1:', 'count_max 2:', 'count_max 6:', 'count_max 1.67772e+07:',
                'count_max - 1', 'two level-4 rows', 'the second the next candidate', 'the second is dropped', 'placed by level 4',
                'NaN, -inf, inf - inf and -0', 'reset byte 0', 'reset byte 1', 'reset byte 2', 'reset byte 255'):
        assert tag in names, tag
    assert {s.slot for s in T} == set(range(22)) and {s.flag for s in T} == {0, 1, 2, 255}
    assert {s.prm for s in T} == set(SC.PARAMS)


def test_scenes(ref):
    """the restatement and float64 WITHOUT probes give every scene's hand-written answer in every word; then the whole table
    through the rule, under half of EDGE_ILL_CAP"""
    T = SC.table()
    wrong = []
    reps = []
    for prm in SC.PARAMS:
        scenes = [s for s in T if s.prm == prm]
        over, P = SC.PARAMS[prm], F.values(**SC.PARAMS[prm])
        bel, see = np.stack([s.prior for s in scenes]), np.stack([s.see for s in scenes])
        flag, slot = np.array([s.flag for s in scenes], dtype=np.uint8), np.array([s.slot for s in scenes])
        assert F.in_domain(bel, see, P), prm
        got = F.restatement(ref, over, bel, see, flag, slot)
        f64, _ = F.update(bel, see, flag, slot % 11, P)
        with np.errstate(over='ignore'):
            f64 = f64.astype(f32)                          # (an exact answer is a float32 number)
        for i, s in enumerate(scenes):
            want = s.answer()
            for who, row in (('restatement', got[i]), ('float64', f64[i])):
                d = SC.same_row(row, want)
                if len(d):
                    wrong.append(f'{s.name} [{prm}]: {who} word {d[0]}: {row[d[0]]!r}, the answer is {want[d[0]]!r} ({len(d)} words differ)')
        rep, fails = F.compare(got, bel, see, flag, slot % 11, P)
        wrong += [f'[{prm}] {f}' for f in fails]
        reps.append(rep)
    assert not wrong, '\n'.join(wrong)
    total = dict(n=sum(r['n'] for r in reps), ill=sum(r['ill'] for r in reps),
                 worst={k: max(r['worst'][k] for r in reps) for k in F.UNIT}, raw={k: max(r['raw'][k] for r in reps) for k in F.UNIT})
    total['share'] = total['ill'] / total['n']
    print(line('scenes', total))
    assert total['n'] == len(T) and total['share'] <= F.EDGE_ILL_CAP / 2, total['share']
    assert total['ill'] >= 5                              # the near-edge scenes do stand on their edges
