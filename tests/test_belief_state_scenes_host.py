"""CPU: the state scenes of tests/belief_state_scenes.py through the host pipeline the cycle kernel is held to: the scene's planes ->
tests/see_ref.c (the see row the device builds, bit for bit) -> the scene's hand-written see facts -> tests/belief_ref.c -> the
hand-written answer in every word (NaN-free, bit for bit, the sign of zero included).  The float64 update of tests/belief_f64.py
without probes gives the same answer; under its probes the `near` scenes are ill-conditioned and the others are not.  The device
runs the same table in tests/test_gpu_match_belief_net_edges.py; the played launches of that file are replayed here on the CPU, which is
where its floors and the ill-conditioned shares come from."""
import numpy as np
import pytest

import belief as B
import belief_f64 as F
import belief_scenes as SC
import belief_state_scenes as SS
import match_see as S

f32 = np.float32
PROBES = 4 * F.K_PROBES                                   # a tie falls the same way in all of K_PROBES probes once in 16 scenes


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('state_scenes')
    return dict(see=S.build(d), bel=B.build(d))


def host_rows(refs, scenes, seed=0x5EED):
    """(prior [R, 192], see [R, 192], flag [R], slot [R]) of the scenes: one match each on a blank state"""
    st = S.blank_state(len(scenes))
    flag = np.array([SS.write_state(st, m, s) for m, s in enumerate(scenes)], dtype=np.uint8)
    rows = S.see(refs['see'], st, S.params(seed=seed, **SS.VISION))
    slot = np.array([s.slot for s in scenes])
    return np.stack([s.prior for s in scenes]), rows[np.arange(len(scenes)), slot], flag, slot


def test_every_bullet_and_edge_is_in_the_table():
    """so that a later edit cannot quietly drop a scene the table is there for"""
    T = SS.table()
    assert {s.bullet for s in T} == set(SS.BULLETS) and len({s.name for s in T}) == len(T)
    assert set(SS.BULLETS) == set(SC.BULLETS) - {'non-finite'}
    names = ' | '.join(s.name for s in T)
    for lv in (1, 2, 3):
        for r in range(21):
            assert f'level {lv}: nearest in row {r} ' in names + ' '
    for tag in ('tie of two, rows 3 and 4', 'tie of two, rows 14 and 15', 'tie of three, rows 2, 6 and 9', 'tie of two, rows 9 and 10',
                'two rows and one entry', 'two rows and two entries', 'a level-4 row names the entry an earlier level-3 row',
                'match_dist = 0: an entry exactly at tol', 'match_dist = 0: an entry one float inside', 'match_dist = 0: an entry one float outside',
                'match_rate = 0: an entry exactly at tol', 'match_rate = 0: an entry one float inside', 'match_rate = 0: an entry one float outside',
                'see_wait 2 of 3: not fresh', 'see_wait 1 of 3: not fresh', 'the agent is sent off', 'ball level 1 keeps', 'ball level 4 takes',
                'inside the cone is forgotten', 'exactly on the cone', 'next float outside the cone', 'a cone of 90 degrees', '(d = 0) is kept',
                'view code 1', 'view code 2', 'view code 3', 'a negative cone', 'the ball as a ghost',
                'count_max 1, fresh', 'count_max 2, fresh', 'count_max 6, fresh', 'count_max 1, not fresh', 'count_max 2, not fresh',
                'count_max 6, not fresh', 'count_max 1: only what this very update saw', 'done byte 0', 'done byte 1', 'done byte 255'):
        assert tag in names, tag
    for slot in range(22):
        assert f'identities seen from slot {slot} (default)' in names and f'identities seen from slot {slot} (other)' in names
        assert f'team word > 0, from slot {slot}:' in names and f'team word < 0, from slot {slot}:' in names
    assert {s.slot % 11 for s in T if s.bullet == 'team word'} >= {0, 5, 10} and {s.slot // 11 for s in T if s.bullet == 'team word'} == {0, 1}
    assert {s.prm for s in T} == set(SS.USED) and {s.slot for s in T} == set(range(22)) and {s.done for s in T} == {0, 1, 255}
    # the counts scenes do hold pos_count = count_max - 2, - 1 and count_max, and counts older than pos_count
    for prm in ('cm1', 'cm2', 'other'):
        cm = SC.count_max(prm)
        for s in (s for s in T if s.bullet == 'counts' and s.prm == prm and 'pos_count' in s.name):
            pc, vc, bc = (s.prior[24 + w::8][:21] for w in (5, 6, 7))
            assert {cm - 1, cm} <= set(pc.tolist()) and (cm < 2 or cm - 2 in pc.tolist())
            assert ((bc > pc) & (pc < cm)).any() and (cm < 2 or ((vc > pc) & (pc < cm)).any())
    # the share of near-edge scenes
    assert sum(s.near for s in T) / len(T) < F.EDGE_ILL_CAP / 2
    # every kind of half-wave, and every divergence between the two halves of a wave in both orders of every launch taken together
    assert {SS.kind(s) for s in T} == {'gate', 'reset', 'none', 'pending'}
    for shift in (0, 1):
        seen = set()
        for prm in SS.USED:
            seen |= SS.divergences([None] * shift + [SS.kind(s) for s in SS.launch_order([s for s in T if s.prm == prm])])
        assert seen == {'can', 'pending', 'reset'}, (shift, seen)


def test_ties_are_bit_equal():
    """the prior rows a tie scene names stand at one and the same fp32 squared distance from the fix (csrc/s2d_device.h: sq2 =
    fmaf(x, x, y * y)), and no other candidate is as near"""
    T = [s for s in SS.table() if s.bullet == 'tie']
    assert len(T) >= 4 and {len(s.ties) for s in T} == {2, 3}
    for s in T:
        low = min(s.ties)
        fx, fy = (f32(v) for v in s.want[1 + low][:2])   # the fix: where the lowest row stands afterwards

        def q(j):
            dx, dy = f32(fx - s.prior[24 + 8 * j]), f32(fy - s.prior[25 + 8 * j])
            return f32(np.float64(dx) * np.float64(dx) + np.float64(f32(np.float64(dy) * np.float64(dy))))
        qs = [q(j) for j in s.ties]
        assert len({v.tobytes() for v in qs}) == 1, (s.name, qs)
        others = [q(j) for j in range(21) if j not in s.ties and s.prior[29 + 8 * j] < s.cm]
        assert others and all(v > qs[0] for v in others), s.name


def test_scenes(refs):
    """see_ref's row holds what the scene states; belief_ref and float64 without probes give the hand-written answer in every word;
    under the probes exactly the near-edge scenes are ill-conditioned"""
    T = SS.table()
    wrong, ill, total = [], 0, 0
    for prm in SS.USED:
        scenes = [s for s in T if s.prm == prm]
        over, P = SS.PARAMS[prm], F.values(**SS.PARAMS[prm])
        bel, see, flag, slot = host_rows(refs, scenes)
        assert not np.isnan(see).any() and not np.isnan(bel).any()
        assert F.in_domain(bel, see, P), prm
        for s, row in zip(scenes, see):
            wrong += [f'{s.name} [{prm}]: the see row: {b}' for b in s.check_see(row)]
        got = F.restatement(refs['bel'], over, bel, see, flag, slot)
        f64, _ = F.update(bel, see, flag, slot % 11, P)
        f64 = f64.astype(f32)                              # (an exact answer is a float32 number)
        rep, fails = F.compare(got, bel, see, flag, slot % 11, P, probes=PROBES)
        wrong += [f'[{prm}] {f}' for f in fails]
        for i, s in enumerate(scenes):
            want = s.answer(see[i])
            assert not np.isnan(want).any()
            for who, row in (('restatement', got[i]), ('float64', f64[i])):
                d = SC.same_row(row, want)
                if len(d):
                    wrong.append(f'{s.name} [{prm}]: {who} word {d[0]}: {row[d[0]]!r}, the answer is {want[d[0]]!r} ({len(d)} words differ)')
            if bool(rep['well'][i]) == bool(s.near):
                wrong.append(f'{s.name} [{prm}]: tagged near = {s.near}, but under the probes it is ' + ('well' if rep['well'][i] else 'ill') + '-conditioned')
        ill, total = ill + rep['ill'], total + rep['n']
        assert max(rep['raw'].values()) == 0.0, (prm, rep['raw'])   # exact scenes: no deviation at all
    assert not wrong, '\n'.join(wrong)
    print(f'state scenes: {total} rows, {ill} ill-conditioned ({100 * ill / total:.3f} %)')
    assert total == len(T) and ill / total < F.EDGE_ILL_CAP / 2 and ill == sum(s.near for s in T)


def test_the_other_agents_do_not_disturb(refs):
    """a scene's row depends on its own match only: the table in launch order and shifted by one match gives the same rows"""
    T = SS.launch_order([s for s in SS.table() if s.prm == 'default'])
    _, a, _, _ = host_rows(refs, T)
    _, b, _, _ = host_rows(refs, T[::-1])
    assert np.array_equal(a.view(np.int32), b[::-1].view(np.int32))


# ------------------------------------------------------------------------------------------------ the played launches, replayed
def replay(tmp, n, T, seed, net, over, prior_cycles=(), prior_seed=None):
    """the host closed loop tests/test_gpu_match_belief_net.py's test_closed_loop_against_the_cpu holds the cycle kernel to (match
    oracle -> see_ref -> belief_ref -> see_policy_ref -> oracle), for the launches of tests/test_gpu_match_belief_net_edges.py's
    parts c and d, kept as single updates: (belief before, see row, flag, slot, belief after) [T * n * 22, ...].  prior_cycles: the
    cycles before which the belief is overwritten with belief_f64.random_rows' priors; then only those cycles' updates are kept."""
    import match_oracle as MO
    import see_policy as SP
    torch = pytest.importorskip('torch')
    from test_gpu_match_see_net import _table
    short = dict(half_time_cycles=10, nr_extra_halfs=0, penalty_shoot_outs=0, after_goal_wait=5)   # test_gpu_match_belief_f64.SHORT
    cfg = MO.make_match_config(seed=seed, noise=1, **short)
    orc = MO.MatchOracle(cfg, n)
    orc.reset()
    see_lib, bel_lib, pol = S.build(tmp), B.build(tmp), SP.build(tmp)
    h1, h2, k, net_seed = net
    torch.manual_seed(net_seed)                            # tests/test_gpu_match_see_policy.py's _module, on the CPU
    m = torch.nn.Sequential(torch.nn.Linear(192, h1), torch.nn.Tanh(), torch.nn.Linear(h1, h2), torch.nn.Tanh(), torch.nn.Linear(h2, k))
    with torch.no_grad():
        m[0].weight[:, [10, 13]] *= 1.0e-4
    params = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    table = _table(k, net_seed)
    vprm, bprm, P = S.params(seed=cfg.seed, env_id_offset=cfg.env_id_offset), B.params(**over), F.values(**over)
    planes = {'neck': np.zeros((n, 24), dtype=f32), 'view_width': np.full((n, 24), 2, dtype=np.int32), 'see_wait': np.zeros((n, 24), dtype=np.int32)}
    bel = B.reset(bel_lib, np.zeros((n, 22, 192), dtype=f32))
    flag = np.zeros(n, dtype=np.uint8)
    gid, slots = np.arange(n) + cfg.env_id_offset, list(range(22))
    rng = None if prior_seed is None else np.random.default_rng(prior_seed)
    rows = []
    for t in range(T):
        if t in prior_cycles:
            bel = F.random_rows(rng, n * 22, P)[0].reshape(n, 22, 192)
        st = dict({key: orc.get(key) for key in S.ENGINE_KEYS}, **planes)
        see = S.see(see_lib, st, vprm)
        after = B.step(bel_lib, bprm, see, bel, flag)
        if not prior_cycles or t in prior_cycles:
            rows.append((bel, see, np.repeat(flag[:, None], 22, axis=1), np.tile(np.arange(22), (n, 1)), after))
        wi, _, _ = SP.actions(pol, after, params, h1, h2, k, True, False, cfg.seed, gid, st['tick'], slots)
        orc.step(np.ascontiguousarray(table[wi][..., :3]))
        flag = orc.get('done').astype(np.uint8)
        planes = S.vision_step(see_lib, dict({key: orc.get(key) for key in S.ENGINE_KEYS}, **planes), vprm,
                               np.ascontiguousarray(table[wi][..., 3:5]), orc.get('done'))
        bel = after
    return [np.concatenate([r[i].reshape((-1,) + r[i].shape[2:]) for r in rows]) for i in range(5)]


def _counts(rep):
    a = rep['disc']['assign']
    return int((a >= 0).sum()), int((a == -1).sum()), int(rep['disc']['ghost'].sum())


def test_reference_replay_figures(tmp_path_factory):
    """Where the floors and caps of tests/test_gpu_match_belief_net_edges.py's parts c and d come from: its launches replayed on the
    CPU from the same seeds, every update held against float64.  The cycle kernel's record must equal these rows bit for bit (that
    file asserts it against belief_ref on its own see rows), so the figures are the cycle kernel's as well; they stand beside the
    scan kernel's in tests/test_belief_f64_host.py.  Measured (this test's output):

        input                       rows   ill-conditioned   assigned  unassigned  ghosts   pos (T 18.32)    vel (T 44.65)    body (T 1.00)
        c. played, 12 x 33          8712    0  (0.000 %)       3061      30960      193    0.34  raw 1.59   0.00  raw 1.49   0.00  raw 1.00
        d. random priors, default   3168    1  (0.032 %)       1695       6673     3742    0.31  raw 1.46   0.00  raw 1.28   0.00  raw 1.00
        d. random priors, other     3168    0  (0.000 %)        565       7815     3553    0.23  raw 1.41   0.00  raw 1.01   0.00  raw 1.00

    c keeps test_played_record's floors (500 / 100 / 100 and a flag), which this launch clears; d's floors are half of what the
    reference gives here.  The ill-conditioned share stays under ILL_CAP / 2 on the host, the device is held to ILL_CAP itself.
    """
    import test_gpu_match_belief_net_edges as G
    tmp = tmp_path_factory.mktemp('replay')
    c = G.PLAYED
    bel, see, flag, slot, got = replay(tmp, c['n'], c['T'], c['seed'], c['net'], {})
    P = F.values()
    assert F.in_domain(bel, see, P) and flag.any()
    rep, fails = F.compare(got, bel, see, flag.reshape(-1), slot.reshape(-1) % 11, P)
    print('c. played', rep['n'], rep['ill'], f"{100 * rep['share']:.3f} %", _counts(rep), rep['worst'], rep['raw'])
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP / 2
    a, u, g = _counts(rep)
    assert a > 500 and u > 100 and g > 100                 # test_played_record's floors hold for this launch
    d = G.PRIORS
    for tag, over in (('default', {}), ('other', G.OTHER)):
        bel, see, flag, slot, got = replay(tmp, d['n'], max(d['cycles']) + 1, d['seed'], d['net'], over, d['cycles'], 50 + len(over))
        P = F.values(**over)
        assert F.in_domain(bel, see, P)
        rep, fails = F.compare(got, bel, see, flag.reshape(-1), slot.reshape(-1) % 11, P)
        print(f'd. random priors, {tag}', rep['n'], rep['ill'], f"{100 * rep['share']:.3f} %", _counts(rep), rep['worst'], rep['raw'])
        assert not fails, fails
        assert rep['share'] <= F.ILL_CAP / 2
        assert all(x > lo for x, lo in zip(_counts(rep), d['floors'][tag])), (_counts(rep), d['floors'][tag])
