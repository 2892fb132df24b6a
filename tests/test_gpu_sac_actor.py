"""The fused SAC actor (s2d_rollout_sac / Engine.rollout_sac, soccer2d_amd.wide_actor.SquashedGaussianActor), every comparison
bit for bit on every record word (action, logp, obs, reward, done, result, terminal_obs, final state, policy_step, statistics):
closed-loop parity against the CPU oracle (the per-step API for the rcssserver noise model) driven by the host restatement
(tests/sac_ref.c) in both modes under the three noise models, at shapes with widths that are no multiples of 16 and with every
activation; chaining; the head against the wide tanh actor; graph replay; independence of the plan; one [256, 256] launch;
rejections with the arena untouched; and the kernel's name."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import sac_ref as S
from test_gpu_ppo_actor import _engine, _kw, _oracle, int32_view, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
nn = torch.nn

DEV = 'cuda:0'
NA = S.NA
ACT = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}
RECORD = ('obs', 'action', 'reward', 'done', 'result', 'logp')
N = 200                      # three full waves and a partial one of 8
SHAPES = ((8,), (64, 64), (20, 12))
ACTS = ('relu', 'tanh', 'sigmoid')


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return S.build(tmp_path_factory.mktemp('sac_ref'))


def _modules(hidden, A, act, seed=0, scale=0.5, ls_bias=-1.0):
    """(latent_pi, mu, log_std) with uniform weights; the raw log-std rows sit around ls_bias"""
    g = torch.Generator().manual_seed(seed)
    layers, win = [], 10
    for w in hidden:
        layers += [nn.Linear(win, w), ACT[act]()]
        win = w
    latent, mu, ls = nn.Sequential(*layers), nn.Linear(win, A), nn.Linear(win, A)
    with torch.no_grad():
        for p in list(latent.parameters()) + list(mu.parameters()) + list(ls.parameters()):
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * scale)
        ls.bias.add_(ls_bias)
    return latent.to(DEV), mu.to(DEV), ls.to(DEV)


def _actor(mods, det=False):
    from soccer2d_amd.wide_actor import SquashedGaussianActor
    return SquashedGaussianActor.from_modules(*mods, device=DEV, deterministic=det)


def _closed_loop_parity(ref, n, T, mode, noise, hidden, act, det=0, warm=3, seed=0x5EED, **kw):
    A = NA[mode]
    eng = _engine(n, mode, noise, seed=seed, **kw)
    orc = _oracle(n, mode, noise, seed=seed, **kw)
    eng.reset(); orc.reset()
    if warm:
        eng.rollout(warm); orc.rollout(warm)
    actor = _actor(_modules(hidden, A, act, seed=n + T + A + len(hidden)), det)
    params = actor.params.cpu().numpy()
    k0 = eng.policy_step.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    out = eng.alloc_rollout(T, terminal_obs=True, logp=True)
    out['terminal_obs'].fill_(float('nan'))
    assert eng.rollout_sac(T, actor, out=out) is out
    torch.cuda.synchronize()
    obs = orc.obs()
    rec = {k: [] for k in RECORD}
    term = np.full((T, n, 10), np.nan, dtype=np.float32)
    for t in range(T):
        a, lp = S.actions(ref, obs, params, hidden, act, mode, det, eng.cfg.seed, k0 + t)
        obs, rew, done, res = orc.step(a)                                    # the env receives the recorded action
        for k, v in (('obs', obs), ('action', a), ('reward', rew), ('done', done), ('result', res), ('logp', lp)):
            rec[k].append(v)
        d = done != 0
        term[t][d] = orc.terminal_obs()[d]
    for k in rec:
        same(out[k], np.stack(rec[k]), f'record.{k}')
    same(out['terminal_obs'], term, 'record.terminal_obs')
    for f in O.STATE_FIELDS:
        if f != 'policy_step':
            same(getattr(eng, f), orc.state(f), f'state.{f}')
    same(eng.policy_step, int32_view(k0 + T), 'policy_step = k0 + T (mod 2^32)')
    same(eng.obs, orc.obs(), 'obs'); same(eng.done, orc.done(), 'done'); same(eng.result, orc.result(), 'result')
    same(eng.reward, rec['reward'][-1], 'reward')
    same(eng.stats[:4], orc.stats()[:4].astype(np.int64), 'stats')
    return out


CASES = [(mode, noise) for mode in ('cont1', 'turn4') for noise in ('off', 'lattice', 'square')]


@pytest.mark.parametrize('mode,noise', CASES)
def test_closed_loop_parity(ref, mode, noise):
    """both modes x three noise models; per case the three shapes, each with another activation, so that the six cases cover
    every (shape, activation) pair twice; max_steps = 5, so every env resets inside T = 12"""
    c = CASES.index((mode, noise))
    for s, hidden in enumerate(SHAPES):
        out = _closed_loop_parity(ref, N, 12, mode, noise, hidden, ACTS[(s + c) % 3], max_steps=5)
        assert int(out['done'].sum()) >= N                                   # auto-resets inside the launch
        a, lp = out['action'].cpu().numpy(), out['logp'].cpu().numpy()
        assert (np.abs(a) <= 1).all() and len(np.unique(a)) > N and np.isfinite(lp).all()


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_closed_loop_parity_deterministic(ref, mode):
    out = _closed_loop_parity(ref, N, 6, mode, 'lattice', (20, 12), 'tanh', det=1, max_steps=5)
    assert (out['action'].abs() <= 1).all()


def test_one_256_256_launch(ref):
    """SB3's default net_arch"""
    _closed_loop_parity(ref, 64, 4, 'turn4', 'lattice', (256, 256), 'relu')


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_chaining(mode):
    """T = 7 then T = 6 equals one launch of T = 13 (continuous: the cached Gaussian block at k & 3 = 3 on entry)"""
    a, b = _engine(N, mode, 'lattice', max_steps=5), _engine(N, mode, 'lattice', max_steps=5)
    a.reset(); b.reset()
    actor = _actor(_modules((20, 12), NA[mode], 'sigmoid', seed=3))
    r1 = {k: v.clone() for k, v in a.rollout_sac(7, actor, terminal_obs=True).items() if v is not None}
    assert int(a.policy_step[0]) & 3 == 3
    r2 = a.rollout_sac(6, actor, terminal_obs=True)
    r = b.rollout_sac(13, actor, terminal_obs=True)
    torch.cuda.synchronize()
    for k in RECORD:
        same(torch.cat([r1[k], r2[k]]), r[k].cpu().numpy(), k)
    d = torch.cat([r1['done'], r2['done']]).bool()
    same(torch.cat([r1['terminal_obs'], r2['terminal_obs']])[d], r['terminal_obs'][d].cpu().numpy(), 'terminal_obs')
    assert torch.equal(a.arena, b.arena)


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_head_equals_the_wide_tanh_actor(mode):
    """log-std rows at -20 (zero weights, bias -30) and the deterministic word set: the action is rollout_actor's on the mean
    rows' network (noise off, epsilon 0), bit for bit"""
    from soccer2d_amd.wide_actor import WideDeterministicActor
    A = NA[mode]
    latent, mu, ls = _modules((20, 12), A, 'tanh', seed=5)
    with torch.no_grad():
        ls.weight.zero_(); ls.bias.fill_(-30.0)
    a, b = _engine(N, mode, 'lattice', max_steps=5), _engine(N, mode, 'lattice', max_steps=5)
    a.reset(); b.reset()
    ra = a.rollout_sac(9, _actor((latent, mu, ls), det=True))
    rb = b.rollout_actor(9, WideDeterministicActor.from_module(nn.Sequential(*latent, mu, nn.Tanh()), device=DEV, epsilon=0.0))
    torch.cuda.synchronize()
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        same(ra[k], rb[k].cpu().numpy(), k)
    assert torch.equal(a.arena, b.arena)
    # z = 0: logp = -(ls) - 0.91893853 - log(1 - a^2 + 1e-6) per dimension, with ls = -20
    lp = ra['logp'].cpu().numpy().astype(np.float64)
    act = ra['action'].cpu().numpy().astype(np.float64)
    assert np.abs(lp - (A * (20 - 0.9189385332) - np.log(1 - act ** 2 + 1e-6).sum(axis=2))).max() < 1e-3


def test_graph_replay_reads_weights_and_the_deterministic_word_at_replay():
    n, T, mode = N, 8, 'turn4'
    eng = _engine(n, mode, 'lattice', max_steps=5)
    eng.reset()
    mods, other = _modules((20, 12), 4, 'tanh', seed=7), _modules((20, 12), 4, 'tanh', seed=8)
    actor = _actor(mods)
    out = eng.alloc_rollout(T, terminal_obs=True, logp=True)
    eng.rollout_sac(T, actor, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.rollout_sac(T, actor, out=out)
    torch.cuda.synchronize()
    for det in (False, True, False):
        with torch.no_grad():                                                # the modules change in place; sync() repacks them
            for p, q in zip([p for m in mods for p in m.parameters()], [p for m in other for p in m.parameters()]):
                p.copy_(q * (1.5 if det else 1.0))
        actor.sync()
        actor.deterministic = det
        sd = eng.state_dict()
        g.replay()
        torch.cuda.synchronize()
        got = {k: out[k].clone() for k in RECORD}
        arena = eng.arena.clone()
        eng.load_state_dict(sd)
        r = eng.rollout_sac(T, _actor(mods, det))
        torch.cuda.synchronize()
        for k in got:
            same(got[k], r[k].cpu().numpy(), f'det={det} {k}')
        assert torch.equal(arena, eng.arena), det


def test_results_do_not_depend_on_the_plan(monkeypatch):
    """S2D_WIDE_PLAN=waves,tiles (read at every launch): every pair that fits gives the same record and arena"""
    from soccer2d_amd.wide_actor import wide_plan
    mode, hidden = 'turn4', (20, 12)
    actor = _actor(_modules(hidden, 4, 'relu', seed=11))
    base = _engine(N, mode, 'lattice', max_steps=5)
    base.reset()
    want = base.rollout_sac(7, actor, terminal_obs=True)
    torch.cuda.synchronize()
    assert base.kernel_name().endswith('waves=%d,tiles=%d>' % wide_plan(hidden, 8)[:2])
    ran = 0
    for waves in (4, 2, 1):
        for tiles in (4, 2, 1):
            if (waves, tiles) == wide_plan(hidden, 8)[:2]:
                continue
            monkeypatch.setenv('S2D_WIDE_PLAN', f'{waves},{tiles}')
            eng = _engine(N, mode, 'lattice', max_steps=5)
            eng.reset()
            try:
                got = eng.rollout_sac(7, actor, terminal_obs=True)
            except ValueError as e:
                assert 'S2D_WIDE_PLAN' in str(e)
                continue
            torch.cuda.synchronize()
            assert eng.kernel_name().endswith(f'waves={waves},tiles={tiles}>'), eng.kernel_name()
            for k in RECORD:
                same(got[k], want[k].cpu().numpy(), f'plan {waves},{tiles} {k}')
            assert torch.equal(eng.arena, base.arena)
            ran += 1
    monkeypatch.delenv('S2D_WIDE_PLAN')
    assert ran >= 5


def test_kernel_name_and_record_forms():
    from soccer2d_amd.vec_env import Soccer2DVecEnv
    from soccer2d_amd.wide_actor import wide_plan
    venv = Soccer2DVecEnv(N, noise_model='rcssserver', **_kw('cont1'))
    venv.reset()
    actor = _actor(_modules((20, 12), 1, 'sigmoid'))
    r = venv.rollout(5, policy=actor, terminal_obs=True)                     # dispatch on the actor's type
    torch.cuda.synchronize()
    assert r['action'].shape == (5, N, 1) and r['terminal_obs'].shape == (5, N, 10) and r['logp'].shape == (5, N)
    waves, tiles = wide_plan((20, 12), 2)[:2]
    assert venv.engine.kernel_name() == (f's2d_wide_sac_rollout_kernel<mode=cont1,noise=2,act=sigmoid,h=20-12,a=2,waves={waves},'
                                         f'tiles={tiles}>')
    eng = _engine(N, 'turn4', 'off')
    eng.reset()
    r = eng.rollout_sac(3, _actor(_modules((8,), 4, 'relu')), logp=False, with_obs=False)
    assert 'logp' not in r and r['obs'] is None
    assert eng.kernel_name().startswith('s2d_wide_sac_rollout_kernel<mode=turn4,noise=0,act=relu,h=8,a=8,')
    out = eng.alloc_rollout(3, logp=True)
    out['logp'] = out['logp'].double()
    with pytest.raises(ValueError):
        eng.rollout_sac(3, _actor(_modules((8,), 4, 'relu')), out=out)


def test_rejections_leave_the_state_unchanged(monkeypatch):
    from soccer2d_amd import _capi
    from soccer2d_amd.wide_actor import SquashedGaussianActor, WideDeterministicActor
    ro = _capi.S2DRollout()
    eps = torch.zeros(1, device=DEV)
    for mode in ('cont1', 'turn4'):
        A = NA[mode]
        actor = _actor(_modules((20, 12), A, 'tanh'))
        eng = _engine(N, mode, 'off')
        eng.reset()
        arena = eng.arena.clone()
        det = actor.deterministic_tensor.data_ptr()

        def refused(what, needle, net=None, T=4, det_ptr=det):
            rc = eng.lib.s2d_rollout_sac(eng._h, T, C.byref(net if net is not None else actor.c_struct()), det_ptr, C.byref(ro), None, None,
                                         eng._stream())
            text = eng.lib.s2d_last_error().decode()
            assert rc == _capi.S2D_EINVAL and 's2d_rollout_sac' in text and needle in text, (mode, what, rc, text)

        def struct(**over):
            net = actor.c_struct()
            for k, v in over.items():
                setattr(net, k, v)
            return net
        refused('n_out = A', 'n_out', struct(n_out=A))
        refused('n_out = 2A + 1', 'n_out', struct(n_out=2 * A + 1))
        bad = struct(); bad.hidden[1] = 10
        refused('a width off the grid', 'hidden', bad)
        refused('n_hidden 6', 'n_hidden', struct(n_hidden=6))
        refused('activation 3', 'activation', struct(activation=3))
        refused('epsilon set', 'epsilon', struct(epsilon=eps.data_ptr()))
        refused('noise set', 'noise', struct(noise=eps.data_ptr()))
        refused('noise_kind 1', 'noise_kind', struct(noise_kind=1))
        refused('params NULL', 'params', struct(params=None))
        refused('params misaligned', 'params', struct(params=actor.params.data_ptr() + 4))
        refused('deterministic NULL', 'deterministic', det_ptr=None)
        refused('deterministic misaligned', 'deterministic', det_ptr=det + 2)
        refused('workspace NULL', 'workspace', struct(workspace=None))
        refused('workspace misaligned', 'workspace', struct(workspace=actor.workspace.data_ptr() + 16))
        refused('workspace small', 'workspace', struct(workspace_bytes=actor.workspace.numel() * 4 - 4))
        refused('n_steps 0', 'n_steps', T=0)
        monkeypatch.setenv('S2D_WIDE_PLAN', '3,1')
        refused('plan', 'S2D_WIDE_PLAN')
        monkeypatch.delenv('S2D_WIDE_PLAN')
        with pytest.raises(ValueError, match='action_dim'):
            eng.rollout_sac(4, _actor(_modules((8,), 5 - A, 'relu')))
        with pytest.raises(ValueError, match='n_steps'):
            eng.rollout_sac(0, actor)
        with pytest.raises(ValueError, match='s2d_rollout_sac'):             # another family's actor
            eng.rollout_sac(4, WideDeterministicActor((8,), A, device=DEV))
        with pytest.raises(ValueError, match='s2d_rollout_actor'):
            eng.rollout_actor(4, actor)
        torch.cuda.synchronize()
        assert torch.equal(arena, eng.arena), mode
    disc = _engine(N, 'discrete', 'off')
    disc.reset()
    arena = disc.arena.clone()
    actor = _actor(_modules((8,), 1, 'relu'))
    rc = disc.lib.s2d_rollout_sac(disc._h, 4, C.byref(actor.c_struct()), actor.deterministic_tensor.data_ptr(), C.byref(ro), None, None,
                                  disc._stream())
    assert rc == _capi.S2D_EINVAL and 'continuous-action engine' in disc.lib.s2d_last_error().decode()
    with pytest.raises(ValueError, match='continuous-action'):
        disc.rollout_sac(4, actor)
    torch.cuda.synchronize()
    assert torch.equal(arena, disc.arena)
    assert isinstance(actor, SquashedGaussianActor)
