"""The opt-in movement-noise model noise_model='rcssserver' (S2DConfig.noise_model = S2D_NOISE_RCSSSERVER): rcssserver's
MPObject::noise() adds (drand(-m, m), drand(-m, m)) with m = rand * |v| to a velocity -- a uniform square, E|dv|^2 = 2 m^2 / 3 and
|dv| > m in 1 - pi / 4 of the draws -- where the default lattice draws polar(U(0, m), whole degree), E|dv|^2 = m^2 / 3, |dv| < m.

  1. the draw (s2d_debug_eval ops 11 / 12) against a restatement of its spec on the oracle's Philox, and its statistics;
  2. the engine's velocity noise has the square's distribution (the lattice fails every one of these checks);
  3. one cycle from injected states = the noiseless CPU oracle + c * rand * |v| with c from op 11;
  4. every entry point computes the same trajectories; 5. the default is the lattice, unchanged; 6. full size; 7. drop-in.
rcssserver's own generator stream cannot be reproduced: what is pinned is the published distribution, not its numbers."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
chi2 = pytest.importorskip('scipy.stats').chi2

P_TAIL = 1e-6
SEED = 0x5EED
PLAYER_RAND, BALL_RAND, PLAYER_DECAY, BALL_DECAY = 0.1, 0.05, 0.4, 0.94   # s2d_default_config (rcssserver stock)
RSUM = 0.3 + 0.085


def _engine(n, **kw):
    from soccer2d_amd.engine import Engine, make_config
    return Engine(n, 'cuda:0', cfg=make_config(server_params=kw.pop('server', None), **kw))


def _lib():
    from soccer2d_amd import _capi
    return _capi, _capi.load_library()


def check_uniform(counts, what):
    counts = np.asarray(counts, dtype=np.float64)
    e = counts.sum() / len(counts)
    stat, dof = float(((counts - e) ** 2 / e).sum()), len(counts) - 1
    assert stat < chi2.isf(P_TAIL, dof), f"{what}: chi2 = {stat:.1f} with {dof} dof"


# ---------------------------------------------------------------- the spec, restated on the host
M32 = np.uint64(0xFFFFFFFF)


def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over numpy arrays (the oracle's O.philox, vectorised; checked against it below)."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = c[0] * np.uint64(0xD2511F53)
        p1 = c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return [x.astype(np.uint32) for x in c]


def square_units(gid_lo, gid_hi, ctr, stream, seed):
    """The spec of the draw: block 2 of `stream` at counter `ctr`; each word w -> (w >> 8) * 2^-24 * 2 - 1 (exact in fp32)."""
    w = philox_np(gid_lo, gid_hi, ctr, (stream << 16) | 2, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack([((x >> np.uint32(8)).astype(np.float64) * 2.0 ** -23 - 1.0).astype(np.float32) for x in w], axis=1)


def device_units(op, gid_lo, gid_hi, ctr, seed_lo):
    _capi, lib = _lib()
    n = len(gid_lo)
    x = np.stack([gid_lo, gid_hi, ctr, np.full(n, seed_lo, np.uint32)], axis=1).astype(np.uint32)
    xt = torch.from_numpy(x.view(np.int32)).cuda().contiguous()
    y = torch.empty((n, 4), dtype=torch.float32, device='cuda:0')
    _capi.check(lib, lib.s2d_debug_eval(op, xt.data_ptr(), y.data_ptr(), n, None), 's2d_debug_eval')
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_numpy_philox_equals_the_oracle():
    rs = np.random.RandomState(1)
    for _ in range(64):
        ctr = [int(v) for v in rs.randint(0, 2 ** 32, 4, dtype=np.uint64)]
        key = [int(v) for v in rs.randint(0, 2 ** 32, 2, dtype=np.uint64)]
        got = [int(v[0]) for v in philox_np([ctr[0]], [ctr[1]], [ctr[2]], [ctr[3]], key[0], key[1])]
        assert got == [int(v) for v in O.philox(ctr, key)]


@pytest.mark.parametrize('op,stream', [(11, 3), (12, 5)])
def test_square_draw_bit_for_bit(op, stream):
    n = 1 << 16
    gid = (np.arange(n, dtype=np.uint64) * 3 + 11).astype(np.uint32)
    hi = np.full(n, 7, np.uint32)
    allv = []
    for k in (0, 1, 6, 7, 1001, 65536 + 3):
        got = device_units(op, gid, hi, np.full(n, k, np.uint32), SEED)
        want = square_units(gid, hi, np.full(n, k, np.uint32), stream, SEED)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (op, k)
        allv.append(got)
    v = np.concatenate(allv).astype(np.float64)
    assert v.min() >= -1.0 and v.max() < 1.0
    assert np.array_equal(v * 2.0 ** 23, np.rint(v * 2.0 ** 23))          # the 2^-23 grid
    for j in range(4):
        check_uniform(np.bincount(((v[:, j] + 1.0) * 32.0).astype(np.int64), minlength=64), f'op {op} component {j}')
    r = np.corrcoef(v.T)
    assert np.abs(r[np.triu_indices(4, 1)]).max() < 0.01, r


def test_square_draw_streams_differ_from_each_other_and_from_the_lattice_block():
    n = 4096
    gid, hi, k = np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32), np.full(n, 5, np.uint32)
    a, b = device_units(11, gid, hi, k, SEED), device_units(12, gid, hi, k, SEED)
    assert (a != b).mean() > 0.99
    assert (device_units(11, gid, hi, k, SEED + 1) != a).mean() > 0.99


# ---------------------------------------------------------------- 2. engine-level distribution
def _noise_samples(steps=4, n=65536):
    """Velocity noise of player (dashing) and ball, isolated one cycle at a time: a noise-off engine is given the noisy engine's
    state before each cycle and the same command, so (v_on - v_off) / decay = dv and |v_off| / decay = |v| after the clamp."""
    from soccer2d_amd import _capi
    kw = dict(use_continuous_action=False, change_ball_velocity=True, auto_reset=False, max_steps=10 ** 6, min_distance_to_ball=0.0)
    on = _engine(n, noise_model='rcssserver', **kw)
    off = _engine(n, noise=False, **kw)
    on.reset()
    rs = np.random.RandomState(3)
    out = {'player': [], 'ball': []}
    for t in range(steps):
        for f in _capi.STATE_FIELDS:
            getattr(off, f).copy_(getattr(on, f))
        cmd = np.zeros((n, 4), np.float32)
        cmd[:, 0], cmd[:, 1], cmd[:, 2] = _capi.CMD_DASH, 100.0, rs.uniform(-180, 180, n)
        on.step_commands(cmd)
        off.step_commands(cmd)
        torch.cuda.synchronize()
        for who, fx, fy, rand, decay in (('player', 'player_vx', 'player_vy', PLAYER_RAND, PLAYER_DECAY),
                                         ('ball', 'ball_vx', 'ball_vy', BALL_RAND, BALL_DECAY)):
            v_on = np.stack([getattr(on, fx).cpu().numpy(), getattr(on, fy).cpu().numpy()]).astype(np.float64)
            v_off = np.stack([getattr(off, fx).cpu().numpy(), getattr(off, fy).cpu().numpy()]).astype(np.float64)
            speed = np.hypot(*v_off) / decay
            far = np.ones(n, bool)
            for e in (on, off):
                d = np.hypot(e.ball_x.cpu().numpy() - e.player_x.cpu().numpy(), e.ball_y.cpu().numpy() - e.player_y.cpu().numpy())
                far &= d > RSUM + 0.1                          # no collision in either run
            ok = far & (speed > 0.3)                           # fast enough for fp32 to resolve the noise
            out[who].append(((v_on - v_off)[:, ok] / decay) / (rand * speed[ok]))
    return {k: np.concatenate(v, axis=1) for k, v in out.items()}


def test_engine_noise_has_the_square_distribution():
    s = _noise_samples()
    for who in ('player', 'ball'):
        u = s[who]
        assert u.shape[1] >= 100000, (who, u.shape)
        assert np.abs(u).max() < 1.0 + 1e-3, who
        for j in range(2):
            check_uniform(np.bincount(np.clip(((u[j] + 1.0) * 10.0).astype(np.int64), 0, 19), minlength=20), f'{who} axis {j}')
        r2 = (u ** 2).sum(axis=0)
        beyond = float((r2 > 1.0).mean())
        assert 0.19 <= beyond <= 0.24, (who, beyond)       # square: 1 - pi / 4 = 0.215; lattice: 0
        m = float(r2.mean())
        assert 0.64 <= m <= 0.69, (who, m)                 # square: 2 / 3; lattice: 1 / 3


# ---------------------------------------------------------------- 3. one cycle against the noiseless CPU oracle
def _random_states(n, rs):
    from soccer2d_amd import _capi
    ang = rs.uniform(0, 2 * np.pi, n)
    dist = rs.uniform(2.0, 20.0, n)
    px, py = rs.uniform(-40, 40, n), rs.uniform(-25, 25, n)
    sp, sd = rs.uniform(0.0, 1.0, n), rs.uniform(-np.pi, np.pi, n)
    bs, bd = rs.uniform(0.0, 2.9, n), rs.uniform(-np.pi, np.pi, n)
    st = dict(player_x=px, player_y=py, player_vx=sp * np.cos(sd), player_vy=sp * np.sin(sd),
              player_body=rs.uniform(-180, 180, n), stamina=rs.uniform(0, 8000, n), effort=rs.uniform(0.6, 1.0, n),
              recovery=rs.uniform(0.5, 1.0, n), stamina_capacity=rs.uniform(0, 130600, n),
              ball_x=px + dist * np.cos(ang), ball_y=py + dist * np.sin(ang), ball_vx=bs * np.cos(bd), ball_vy=bs * np.sin(bd),
              prev_dist=dist, prev_angle=rs.uniform(-180, 180, n),
              step_number=rs.randint(0, 100, n), cycle=rs.randint(0, 10 ** 6, n), policy_step=rs.randint(0, 10 ** 6, n),
              episode=rs.randint(1, 1000, n))
    return {f: (np.asarray(st[f], np.float32) if i < 15 else np.asarray(st[f], np.int32)) for i, f in enumerate(_capi.STATE_FIELDS)}


def _inject(eng, st):
    for f, v in st.items():
        getattr(eng, f).copy_(torch.from_numpy(v))


def _oracle_with(st, n, **kw):
    from soccer2d_amd import _capi
    orc = O.OracleEngine(O.make_config(noise=0, auto_reset=0, **kw), n, 'f32')
    rows = np.stack([st[f].astype(np.float64) for f in _capi.STATE_FIELDS], axis=1)
    for i in range(n):
        assert orc.L.s2do_set_env(orc.h, i, O._dp(np.ascontiguousarray(rows[i]))) == 0
    return orc


def test_one_cycle_equals_noiseless_oracle_plus_the_draw():
    from soccer2d_amd import _capi
    n = 4096
    kw = dict(use_continuous_action=False, max_steps=10 ** 6, min_distance_to_ball=0.0)
    rs = np.random.RandomState(11)
    st = _random_states(n, rs)
    cmd = np.zeros((n, 4), np.float32)
    dash = rs.rand(n) < 0.6
    cmd[dash, 0] = _capi.CMD_DASH
    cmd[:, 1] = rs.uniform(-100, 100, n)
    cmd[:, 2] = rs.uniform(-180, 180, n)
    eng = _engine(n, noise_model='rcssserver', auto_reset=False, **kw)
    _inject(eng, st)
    eng.step_commands(cmd)
    torch.cuda.synchronize()
    orc = _oracle_with(st, n, **kw)
    orc.step_commands(cmd)
    g = {f: getattr(eng, f).cpu().numpy() for f in _capi.STATE_FIELDS}
    o = {f: orc.state(f) for f in _capi.STATE_FIELDS}
    c = device_units(11, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32), st['policy_step'].astype(np.uint32), SEED)
    keep = np.ones(n, bool)
    for s in (g, o):
        keep &= np.hypot(s['ball_x'] - s['player_x'], s['ball_y'] - s['player_y']) > RSUM + 0.05
    assert keep.mean() > 0.95
    for f in ('player_body', 'stamina', 'effort', 'recovery', 'stamina_capacity'):
        assert np.array_equal(g[f][keep].view(np.int32), o[f][keep].view(np.int32)), f
    assert np.array_equal(g['policy_step'], st['policy_step'] + 1)
    for who, (fx, fy, vx, vy), rand, decay, cx in (
            ('player', ('player_x', 'player_y', 'player_vx', 'player_vy'), PLAYER_RAND, PLAYER_DECAY, 0),
            ('ball', ('ball_x', 'ball_y', 'ball_vx', 'ball_vy'), BALL_RAND, BALL_DECAY, 2)):
        speed = np.hypot(o[vx].astype(np.float64), o[vy].astype(np.float64)) / decay   # |v| after the clamp, before the noise
        for axis, (fp, fv) in enumerate(((fx, vx), (fy, vy))):
            d = c[:, cx + axis].astype(np.float64) * rand * speed
            # (the scale of a few ulp: the largest of the two results and the velocity that was added up)
            for got, base, delta, v in ((g[fp], o[fp], d, speed), (g[fv], o[fv], decay * d, decay * speed)):
                got, base = got.astype(np.float64), base.astype(np.float64)
                want = base + delta
                scale = np.maximum(np.maximum(np.abs(got), np.abs(base)), v).astype(np.float32)
                tol = 4 * np.spacing(scale).astype(np.float64) + 1e-5 * np.abs(delta)
                err = np.abs(got - want)
                bad = keep & (err > tol)
                assert not bad.any(), (who, fp, fv, int(bad.sum()), float((err - tol)[bad].max()))
    # turns: the turn noise is the same draw in both models, so the body equals the lattice engine's from the same state
    cmd[:, 0] = _capi.CMD_TURN
    bodies = []
    for model in ('rcssserver', 'lattice'):
        e = _engine(n, noise_model=model, auto_reset=False, **kw)
        _inject(e, st)
        e.step_commands(cmd)
        torch.cuda.synchronize()
        bodies.append(e.player_body.cpu().numpy())
    assert np.array_equal(bodies[0].view(np.int32), bodies[1].view(np.int32))
    assert (bodies[0] != st['player_body']).mean() > 0.9


# ---------------------------------------------------------------- 4. entry points agree bit for bit
CASES = {
    'discrete': dict(use_continuous_action=False),
    'continuous': dict(use_continuous_action=True),
    'turning': dict(use_continuous_action=True, use_turning=True),
    'random': dict(use_continuous_action=False),
}
BASE = dict(noise_model='rcssserver', change_ball_velocity=True, max_steps=24, min_distance_to_ball=4.0)


def _actions(name, T, n, rs):
    if name == 'random':
        return None
    if name == 'discrete':
        return torch.from_numpy(rs.randint(0, 16, (T, n)).astype(np.int32)).cuda()
    if name == 'continuous':
        return torch.from_numpy(rs.uniform(-1, 1, (T, n, 1)).astype(np.float32)).cuda()
    return torch.from_numpy(rs.uniform(-1, 1, (T, n, 4)).astype(np.float32)).cuda()


def _state(eng):
    from soccer2d_amd import _capi
    return {f: getattr(eng, f).cpu().numpy().copy() for f in _capi.STATE_FIELDS}


def _run(path, name, n, T, acts):
    eng = _engine(n, **BASE, **CASES[name])
    eng.reset()
    rec = {k: [] for k in ('obs', 'reward', 'done', 'result')}
    if path == 'step':
        for t in range(T):
            obs, rew, done, res = eng.step(None if acts is None else acts[t])
            for k, v in (('obs', obs), ('reward', rew), ('done', done), ('result', res)):
                rec[k].append(v.clone())
        rec = {k: torch.stack(v) for k, v in rec.items()}
    elif path == 'step_k':
        for t in range(0, T, 4):
            out = eng.step_k(4, None if acts is None else acts[t:t + 4].contiguous())
            for k in rec:
                rec[k].append(out[k].clone())
        rec = {k: torch.cat(v) for k, v in rec.items()}
    else:
        out = eng.rollout(T, acts)
        rec = {k: out[k].clone() for k in rec}
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in rec.items()}, _state(eng), eng.kernel_name()


def _same(a, b, what):
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape, (what, k)
        if x.dtype == np.float32:
            x, y = x.view(np.int32), y.view(np.int32)
        assert np.array_equal(x, y), (what, k, int((x != y).sum()))


@pytest.mark.parametrize('n', [777, 4096])
@pytest.mark.parametrize('name', sorted(CASES))
def test_entry_points_agree(name, n, monkeypatch):
    T = 64
    acts = _actions(name, T, n, np.random.RandomState(n))
    ref_rec, ref_state, _ = _run('step', name, n, T, acts)
    assert ref_rec['done'].sum() > n // 2                  # resets inside the run
    rec, st, _ = _run('step_k', name, n, T, acts)
    _same(ref_rec, rec, 'step_k'); _same(ref_state, st, 'step_k state')
    for ws, kern in (('1', 's2d_reach_rollout_ws_kernel<'), ('0', 's2d_reach_rollout_kernel<')):
        monkeypatch.setenv('S2D_ROLLOUT_WS', ws)
        rec, st, kname = _run('rollout', name, n, T, acts)
        assert kname.startswith(kern) and 'noise=2' in kname, kname
        _same(ref_rec, rec, f'rollout ws={ws}'); _same(ref_state, st, f'rollout ws={ws} state')
    # the two-envs-per-lane pipeline has no rcssserver model: S2D_ROLLOUT_E=2 falls back to the four-wave kernel
    monkeypatch.setenv('S2D_ROLLOUT_WS', '1')
    monkeypatch.setenv('S2D_ROLLOUT_E', '2')
    rec, st, kname = _run('rollout', name, n, T, acts)
    assert kname.startswith('s2d_reach_rollout_ws_kernel<') and 'noise=2' in kname, kname
    _same(ref_rec, rec, 'rollout E=2'); _same(ref_state, st, 'rollout E=2 state')


# ---------------------------------------------------------------- 5. the default did not move
@pytest.mark.parametrize('ws', ['1', '0'])
def test_default_is_the_lattice(ws, monkeypatch):
    monkeypatch.setenv('S2D_ROLLOUT_WS', ws)
    n, T = 4096, 64
    kw = dict(use_continuous_action=False, change_ball_velocity=True)
    runs = {}
    for key, extra in (('default', {}), ('lattice', dict(noise_model='lattice')), ('rcssserver', dict(noise_model='rcssserver'))):
        eng = _engine(n, **kw, **extra)
        eng.reset()
        out = eng.rollout(T)
        eng.step(None)
        torch.cuda.synchronize()
        runs[key] = ({k: v.cpu().numpy() for k, v in out.items()}, _state(eng), eng.kernel_name())
    d, lat, rc = runs['default'], runs['lattice'], runs['rcssserver']
    _same(d[0], lat[0], 'record'); _same(d[1], lat[1], 'state')
    eng = _engine(n, **kw)
    eng.reset(); eng.rollout(T)
    kname = eng.kernel_name()
    if ws == '1':
        assert kname.startswith('s2d_reach_rollout_ws_kernel<discrete,noise=1,'), kname
    else:
        assert kname == 's2d_reach_rollout_kernel<discrete,noise=1>', kname
    assert not np.array_equal(d[1]['player_x'], rc[1]['player_x'])


# ---------------------------------------------------------------- 6. full size
def test_full_size():
    n, T = 65536, 256
    kw = dict(noise_model='rcssserver', use_continuous_action=False, change_ball_velocity=True)

    def run(seed):
        eng = _engine(n, seed=seed, **kw)
        eng.reset()
        out = eng.rollout(T)
        torch.cuda.synchronize()
        return eng, {k: v.cpu().numpy() for k, v in out.items()}
    eng, rec = run(SEED)
    assert all(v == 0 for v in eng.validate_state().values()), eng.validate_state()
    assert np.isfinite(rec['obs']).all() and np.isfinite(eng.obs.cpu().numpy()).all()
    resets = rec['done'].sum(axis=0).astype(np.int64)
    assert resets.sum() > n
    assert np.array_equal(eng.cycle.cpu().numpy(), T + 1 + resets)
    assert np.array_equal(eng.episode.cpu().numpy(), 1 + resets)
    _, rec2 = run(SEED)
    _same(rec, rec2, 'same seed')
    _, rec3 = run(SEED + 1)
    assert not np.array_equal(rec['obs'], rec3['obs'])
    sd = eng.state_dict()
    a = eng.rollout(32)
    a = {k: v.cpu().numpy() for k, v in a.items()}
    eng.load_state_dict(sd)
    b = eng.rollout(32)
    _same(a, {k: v.cpu().numpy() for k, v in b.items()}, 'state_dict round trip')


# ---------------------------------------------------------------- 7. drop-in surfaces
def test_dropin_surfaces_take_the_model():
    from sample_environments.reach_ball_env import ReachBallEnv
    from soccer2d_amd import _capi
    from soccer2d_amd.hook_env import HookVecEnv
    from soccer2d_amd.sb3_vec_env import S2DSB3VecEnv
    from soccer2d_amd.vec_env import Soccer2DVecEnv
    from hook_reach_ball import HookReachBall
    env = ReachBallEnv(noise_model='rcssserver', use_continuous_action=False)
    assert env.vec.engine.cfg.noise_model == _capi.NOISE_RCSSSERVER
    obs = env.reset()
    for t in range(30):
        obs, r, done, info = env.step(t % 16)
        if done:
            obs = env.reset()
    assert np.isfinite(obs).all()
    env.close()
    assert ReachBallEnv(use_continuous_action=False).vec.engine.cfg.noise_model == _capi.NOISE_LATTICE
    venv = S2DSB3VecEnv(64, noise_model='rcssserver', use_continuous_action=False)
    assert venv.venv.engine.cfg.noise_model == _capi.NOISE_RCSSSERVER
    venv.reset()
    for _ in range(5):
        o, r, d, infos = venv.step(np.random.RandomState(0).randint(0, 16, 64))
    assert o.shape == (64, 10) and np.isfinite(o).all()
    venv.close()
    hv = HookVecEnv(HookReachBall, 2, noise_model='rcssserver')
    assert hv.runtime.engine.cfg.noise_model == _capi.NOISE_RCSSSERVER
    hv.reset()
    hv.step([0, 1])
    hv.close()
    with pytest.raises(ValueError):
        Soccer2DVecEnv(4, noise=False, noise_model='rcssserver')


def test_state_dict_refuses_the_other_model():
    kw = dict(use_continuous_action=False)
    a, b = _engine(256, noise_model='rcssserver', **kw), _engine(256, **kw)
    a.reset(); a.rollout(8)
    sd = a.state_dict()
    with pytest.raises(ValueError, match='different engine configuration'):
        b.load_state_dict(sd)
    c = _engine(256, noise_model='rcssserver', **kw)
    c.load_state_dict(sd)
    torch.cuda.synchronize()
    assert torch.equal(c.arena, a.arena)
