"""CPU checks of the fused DDPG / TD3 update's host side (s2d_learn_critic / s2d_learn_actor, soccer2d_amd.learn.ActorCriticLearner):
the ABI additions, the workspace arithmetic, and the host restatement tests/learn_ac_ref.c -- its forward passes against td_ref.c
bitwise, its gradients against float64 torch autograd of the example's losses, a hand-computed case for the tanh head and the -1/B
delta, a training sanity run -- and the argument checks of the class that raise before any library call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import learn as LR
import learn_ac as AC
import td as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('learn_ac_ref')
    return AC.build(d), TD.build(d)


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_additions(tmp_path):
    """the ABI version stays 4, the structs are unchanged, S2D_LEARN_SQUARE is 2 and the header declares the five functions"""
    from soccer2d_amd import _capi, learn
    prog = tmp_path / 'learn_ac_abi.c'
    # sizeof of a function's address is unevaluated: the declarations are checked, nothing is linked
    prog.write_text('#include <stdio.h>\n#include "s2d.h"\nint main(){printf("%d %d %zu %zu %zu", S2D_ABI_VERSION, S2D_LEARN_SQUARE, '
                    'sizeof(S2DLearnNet), sizeof(S2DLearnState), sizeof &s2d_learn_critic + sizeof &s2d_learn_critic_grad + '
                    'sizeof &s2d_learn_actor + sizeof &s2d_learn_actor_grad + sizeof &s2d_learn_actor_workspace_bytes);return 0;}\n')
    exe = tmp_path / 'learn_ac_abi'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [4, 2, C.sizeof(_capi.S2DLearnNet), C.sizeof(_capi.S2DLearnState), 5 * C.sizeof(C.c_void_p)]
    assert learn.AC_LOSSES.index('square') == 2 and learn.AC_LOSSES[:2] == learn.LOSSES and AC.LOSS == {k: i for i, k in enumerate(learn.AC_LOSSES)}


def _shape(n_in, hidden, n_out, act=0):
    from soccer2d_amd import _capi
    s = _capi.S2DLearnNet()
    s.n_in, s.n_hidden, s.n_out, s.activation = n_in, len(hidden), n_out, act
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    return s


def test_symbols_exported_and_workspace_arithmetic():
    """the built library exports and binds the five symbols; s2d_learn_actor_workspace_bytes (host only) agrees with the Python
    arithmetic on the grid and is 0 off it; the critic's workspace is s2d_learn_workspace_bytes of its shape"""
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    from soccer2d_amd.learn import learn_actor_workspace_bytes, learn_param_count, learn_workspace_bytes
    lib = _capi.load_library()
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    for name, nargs in (('s2d_learn_critic', 11), ('s2d_learn_critic_grad', 11), ('s2d_learn_actor', 8), ('s2d_learn_actor_grad', 8),
                        ('s2d_learn_actor_workspace_bytes', 3)):
        assert hasattr(lib, name) and len(protos[name][2]) == nargs, name
    assert protos['s2d_learn_actor_workspace_bytes'][1] is C.c_size_t and _capi.S2D_ABI_VERSION == 4

    def ws(D, A, ha, hc, B):
        return lib.s2d_learn_actor_workspace_bytes(C.byref(_shape(D, ha, A)), C.byref(_shape(D + A, hc, 1)), B)
    for D, A, ha, hc, _ in AC.SHAPES + [(248, 8, (256,) * 4, (256,) * 4, 'relu'), (10, 1, (256, 256), (64,), 'relu')]:
        for B in (1, 63, 64, 65, 4096, 2 ** 31 - 1):
            got = ws(D, A, ha, hc, B)
            assert got == learn_actor_workspace_bytes(D, ha, A, hc, B) and got >= 4 * learn_param_count(D, ha, A), (D, A, ha, hc, B)
            assert got >= learn_workspace_bytes(D, ha, A, B)                 # never less than the actor alone would need
    # reach-ball's pair fits the LDS; 64 rows of the widest pair do not: its images are in the workspace
    assert ws(10, 1, (64, 64), (64, 64), 64) == learn_workspace_bytes(10, (64, 64), 1, 64)
    assert ws(248, 8, (256, 256), (256, 256), 64) > 4 * (learn_param_count(248, (256, 256), 8) + 64 * (256 + 4 * 256 + 9))
    # a pair whose networks fit the LDS one by one but not together
    assert learn_workspace_bytes(10, (256, 32), 1, 64) == ws(10, 1, (256, 32), (8,), 64) < ws(10, 1, (256, 32), (256, 128), 64)
    for a, c in ((_shape(10, (64,), 0), _shape(10, (64,), 1)), (_shape(10, (64,), 9), _shape(19, (64,), 1)),
                 (_shape(249, (64,), 1), _shape(250, (64,), 1)), (_shape(10, (64,), 1), _shape(12, (64,), 1)),
                 (_shape(10, (64,), 1), _shape(11, (64,), 2)), (_shape(10, (12,), 1), _shape(11, (64,), 1)),
                 (_shape(10, (64,), 1), _shape(11, (64,) * 5, 1)), (_shape(10, (64,), 1, act=3), _shape(11, (64,), 1))):
        assert lib.s2d_learn_actor_workspace_bytes(C.byref(a), C.byref(c), 64) == 0
    good = (_shape(10, (64,), 1), _shape(11, (64,), 1))
    assert lib.s2d_learn_actor_workspace_bytes(None, C.byref(good[1]), 64) == 0 == lib.s2d_learn_actor_workspace_bytes(C.byref(good[0]), None, 64)
    for B in (0, -1, 2 ** 31):
        assert lib.s2d_learn_actor_workspace_bytes(C.byref(good[0]), C.byref(good[1]), B) == 0
    assert lib.s2d_learn_actor_workspace_bytes(C.byref(good[0]), C.byref(good[1]), 1) > 0


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('shape', AC.SHAPES, ids=AC.shape_id)
def test_forward_equals_td_ref(refs, shape):
    """the critic step's q is td_ref.c's forward of [obs | action], and the actor step's action and q are td_ref.c's td_target_ac
    with next_obs = obs, bit for bit, edge rows included"""
    L, T = refs
    D, A, ha, hc, act = shape
    rs = np.random.RandomState(3)
    actor, critic = AC.random_pair(rs, D, A, ha, hc, act)
    obs, action, target, _ = AC.random_batch(rs, critic, A, 70)
    obs[0] = 0.0
    obs[1] = -0.0
    obs[2] = 1e30
    obs[3, 0] = np.nan
    got = AC.critic_grad(L, critic, 'square', obs, action, target)
    assert np.array_equal(TD.bits(got['q']), TD.bits(TD.forward(T, critic, np.concatenate([obs, action], 1))[:, 0]))
    got = AC.actor_grad(L, actor, critic, obs)
    _, q, a = TD.target_ac(T, actor, critic, None, obs, np.zeros(70, F), np.ones(70, F))
    assert np.array_equal(TD.bits(got['action']), TD.bits(a)) and np.array_equal(TD.bits(got['q']), TD.bits(q))


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('loss', ['square', 'mse', 'huber'])
@pytest.mark.parametrize('shape', AC.SHAPES, ids=AC.shape_id)
def test_critic_gradient_against_float64_autograd(refs, shape, loss, weighted):
    """the restated critic gradient against float64 torch autograd of the example's loss (F.mse_loss for 'square'): at most 4 x the
    largest error of torch's own fp32 autograd on the same inputs, the bound computed here.  B = 150: three blocks, the last partial."""
    L, _ = refs
    D, A, ha, hc, act = shape
    rs = np.random.RandomState(11)
    _, critic = AC.random_pair(rs, D, A, ha, hc, act)
    obs, action, target, weight = AC.random_batch(rs, critic, A, 150)
    if not weighted:
        weight = None
    g64, l64 = AC.torch_critic_grad(critic, loss, obs, action, target, weight, torch.float64)
    g32, l32 = AC.torch_critic_grad(critic, loss, obs, action, target, weight, torch.float32)
    got = AC.critic_grad(L, critic, loss, obs, action, target, weight)
    err_torch, err_ref = np.abs(g32 - g64).max(), np.abs(got['grad'].astype(np.float64) - g64).max()
    print(f'grad error vs float64: torch fp32 {err_torch:.3e}, learn_ac_ref {err_ref:.3e}; |g|max {np.abs(g64).max():.3e}')
    assert err_torch > 0 and err_ref <= 4 * err_torch
    lerr_torch, lerr_ref = abs(l32 - l64), abs(float(got['stats'][0]) - l64)
    print(f'loss error vs float64: torch fp32 {lerr_torch:.3e}, learn_ac_ref {lerr_ref:.3e}')
    # the loss is a sequential fp32 sum of B non-negative terms: to torch's error (its sum is pairwise) the worst case of that
    # order is added, (B - 1) u sum|t| with u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)
    assert lerr_ref <= 4 * max(lerr_torch, np.spacing(F(abs(l64))) / 2) + 149 * 2.0 ** -24 * abs(l64)
    norm64 = np.sqrt((g64 ** 2).sum())
    assert abs(float(got['stats'][1]) - norm64) <= 4 * max(err_torch, np.spacing(F(norm64))) and float(got['stats'][2]) == 1.0
    q64 = TD.forward64(critic, np.concatenate([obs, action], 1))[:, 0]
    assert np.abs(got['td_abs'] - np.abs(q64 - target)).max() < 1e-4


@pytest.mark.parametrize('shape', AC.SHAPES + [(10, 1, (64, 64), (64, 64), ('tanh', 'relu'))], ids=lambda s: AC.shape_id(s[:4] + (''.join(s[4]),)))
def test_actor_gradient_against_float64_autograd(refs, shape):
    """the restated actor gradient against float64 torch autograd of -q(cat(o, mu(o))).mean(), the same 4 x bound; the critic's
    gradient -- which torch does produce, and which is not zero -- has no array in the restated step, and the critic's parameters
    are bitwise what they were after the gradient call and after a step"""
    L, _ = refs
    D, A, ha, hc, act = shape
    act_a, act_c = act if isinstance(act, tuple) else (act, act)
    rs = np.random.RandomState(13)
    actor, critic = AC.random_pair(rs, D, A, ha, hc, act_a, act_c)
    obs = rs.uniform(-1, 1, (150, D)).astype(F)
    g64, gc64, l64 = AC.torch_actor_grad(actor, critic, obs, torch.float64)
    g32, _, l32 = AC.torch_actor_grad(actor, critic, obs, torch.float32)
    before = critic.params.copy()
    got = AC.actor_grad(L, actor, critic, obs)
    err_torch, err_ref = np.abs(g32 - g64).max(), np.abs(got['grad'].astype(np.float64) - g64).max()
    print(f'grad error vs float64: torch fp32 {err_torch:.3e}, learn_ac_ref {err_ref:.3e}; |g|max {np.abs(g64).max():.3e}')
    assert err_torch > 0 and err_ref <= 4 * err_torch
    lerr_torch, lerr_ref = abs(l32 - l64), abs(float(got['stats'][0]) - l64)
    # -mean q as a sequential fp32 sum: torch's error plus that order's worst case (B - 1) u sum|q| / B, as for the critic's loss
    assert lerr_ref <= 4 * max(lerr_torch, np.spacing(F(abs(l64))) / 2) + 149 * 2.0 ** -24 * np.abs(got['q']).mean()
    norm64 = np.sqrt((g64 ** 2).sum())
    assert abs(float(got['stats'][1]) - norm64) <= 4 * max(err_torch, np.spacing(F(norm64))) and float(got['stats'][2]) == 1.0
    assert got['grad'].size == actor.params.size and np.abs(gc64).max() > 0
    a0 = actor.params.copy()
    AC.actor_step(L, actor, critic, LR.State(actor.params.size, lr=1e-2), obs)
    assert np.array_equal(TD.bits(critic.params), TD.bits(before)) and not np.array_equal(actor.params, a0)


def _hand_pair():
    """actor 1-8-1 ReLU: z = 0.5 relu(x); critic 2-8-1 ReLU: q = 3 relu(2 a) + 0.25 (it reads the action column alone)"""
    e0 = np.eye(8, dtype=F)[0]
    actor = TD.Net(1, (8,), 1, 'relu', np.concatenate([e0, np.zeros(8), 0.5 * e0, [0.0]]).astype(F))
    W1 = np.zeros((8, 2), F)
    W1[0, 1] = 2.0
    critic = TD.Net(2, (8,), 1, 'relu', np.concatenate([W1.ravel(), np.zeros(8), 3 * e0, [0.25]]).astype(F))
    return actor, critic


def test_hand_computed_tanh_head_and_delta(refs):
    """B = 2, obs 1 and -1.  Row 0: a = tanh(0.5), q = 6 a + 0.25; the critic's output delta is -1/2, its unit's delta 3 (-1/2), the
    action column's s = 2 (-3/2) = -3 and dz = -3 (1 - a a).  Row 1: a = 0 and the critic's unit sits at exactly 0, so nothing
    flows.  Every product below is exact in fp32 given a."""
    L, _ = refs
    actor, critic = _hand_pair()
    obs = np.array([[1.0], [-1.0]], F)
    got = AC.actor_grad(L, actor, critic, obs)
    a = got['action'][0, 0]
    assert abs(float(a) - np.tanh(0.5)) < 1e-6 and TD.bits(got['action'][1, 0]) == 0
    assert np.array_equal(got['q'], np.array([F(6) * a + F(0.25), 0.25], F))
    dz = F(-3.0) * (F(1.0) - a * a)
    e0 = np.eye(8, dtype=F)[0]
    want = np.concatenate([F(0.5) * dz * e0, F(0.5) * dz * e0, dz * e0, [dz]]).astype(F)
    assert np.array_equal(got['grad'], want), (got['grad'], want)
    assert got['stats'][0] == -(got['q'][0] + got['q'][1]) / F(2) and got['stats'][1] == np.sqrt(F(F(0.5) * dz * dz + F(2) * dz * dz))
    g64, _, l64 = AC.torch_actor_grad(actor, critic, obs, torch.float64)
    assert np.abs(g64 - want).max() < 1e-6 and abs(l64 - float(got['stats'][0])) < 1e-6
    # the critic's three losses on the same pair: e = q - target = 2 in row 0, 0 in row 1
    action = got['action']
    target = np.array([got['q'][0] - F(2), 0.25], F)
    for loss, d, l in (('square', 4.0, 4.0), ('mse', 2.0, 2.0), ('huber', 1.0, 1.5)):
        c = AC.critic_grad(L, critic, loss, obs, action, target)
        assert np.array_equal(c['td_abs'], np.array([2.0, 0.0], F)) and float(c['stats'][0]) == l / 2
        assert float(c['grad'][-1]) == d / 2 and c['grad'][24] == F(d / 2) * (F(2) * a)      # db_out; dW_out[0] = delta y_0


def test_training_sanity(refs):
    """200 critic steps on a fixed teacher regression bring the loss under a tenth of its start, then 200 actor steps through the
    trained critic raise mean Q(o, mu(o)) on a fixed batch; torch's fp32 chain on the same batches meets both conditions first, so
    the inputs are known learnable"""
    L, _ = refs
    rs = np.random.RandomState(1)
    D, A, B, lr = 10, 2, 256, 1e-2
    teacher = TD.random_net(rs, D + A, (16, 16), 1, 'tanh', gain=2.0)
    actor, critic = AC.random_pair(rs, D, A, (16, 16), (16, 16), 'tanh')
    batches = []
    for _ in range(200):
        obs, action = rs.uniform(-1, 1, (B, D)).astype(F), rs.uniform(-1, 1, (B, A)).astype(F)
        batches.append((obs, action, TD.forward64(teacher, np.concatenate([obs, action], 1))[:, 0].astype(F)))
    fixed = torch.from_numpy(batches[0][0])
    mu, q = LR.torch_module(actor, torch.float32), LR.torch_module(critic, torch.float32)
    opt_q, opt_mu = torch.optim.Adam(q.parameters(), lr=lr), torch.optim.Adam(mu.parameters(), lr=lr)
    tl, tq = [], []
    for obs, action, target in batches:
        loss = nn.functional.mse_loss(q(torch.from_numpy(np.concatenate([obs, action], 1))).squeeze(1), torch.from_numpy(target))
        opt_q.zero_grad()
        loss.backward()
        opt_q.step()
        tl.append(float(loss.detach()))
    for _ in range(200):
        loss = -q(torch.cat([fixed, torch.tanh(mu(fixed))], 1)).mean()
        opt_mu.zero_grad()
        loss.backward()
        opt_mu.step()
        tq.append(-float(loss.detach()))
    assert np.mean(tl[-10:]) < 0.1 * tl[0] and tq[-1] > tq[0] + 0.1, (tl[0], np.mean(tl[-10:]), tq[0], tq[-1])
    sc, sa, rl, rq = LR.State(critic.params.size, lr=lr, max_grad_norm=0.0), LR.State(actor.params.size, lr=lr, max_grad_norm=0.0), [], []
    for obs, action, target in batches:
        rl.append(float(AC.critic_step(L, critic, sc, 'square', obs, action, target)['stats'][0]))
    for _ in range(200):
        rq.append(-float(AC.actor_step(L, actor, critic, sa, batches[0][0])['stats'][0]))
    print(f'critic loss: torch {tl[0]:.4f} -> {np.mean(tl[-10:]):.4f}, learn_ac_ref {rl[0]:.4f} -> {np.mean(rl[-10:]):.4f}; '
          f'mean q: torch {tq[0]:.4f} -> {tq[-1]:.4f}, learn_ac_ref {rq[0]:.4f} -> {rq[-1]:.4f}')
    assert abs(rl[0] - tl[0]) < 1e-5 and np.mean(rl[-10:]) < 0.1 * rl[0]
    assert abs(np.mean(rl[-10:]) - np.mean(tl[-10:])) < 0.25 * np.mean(tl[-10:])
    assert rq[-1] > rq[0] + 0.1 and abs(rq[-1] - tq[-1]) < 0.25 * (tq[-1] - tq[0])


# ------------------------------------------------------------------------------------------------------- ActorCriticLearner
def seq(n_in, hidden, n_out, act=nn.ReLU, bias=True, head=False):
    layers, win = [], n_in
    for w in hidden:
        layers += [nn.Linear(win, w, bias=bias), act()]
        win = w
    return nn.Sequential(*layers, nn.Linear(win, n_out, bias=bias), *([nn.Tanh()] if head else []))


def test_module_parameters_become_views():
    from soccer2d_amd.learn import ActorCriticLearner, learn_param_count
    mu, q, q2 = seq(10, (64, 64), 1, head=True), seq(11, (64, 64), 1), seq(11, (32,), 1, act=nn.Tanh)
    before = [[p.detach().clone() for p in m.parameters()] for m in (mu, q, q2)]
    lrn = ActorCriticLearner.from_modules(mu, q, q2, actor_lr=3e-4, device='cpu')
    for net, mod, old, P in zip((lrn.actor,) + lrn.critics, (mu, q, q2), before, (learn_param_count(10, (64, 64), 1),
                                                                                 learn_param_count(11, (64, 64), 1), learn_param_count(11, (32,), 1))):
        assert net.params.numel() == P
        off = net.params.data_ptr()
        for p, b in zip(mod.parameters(), old):
            assert p.data_ptr() == off and torch.equal(p.detach(), b)        # nn.Sequential order, values kept
            off += 4 * p.numel()
    with torch.no_grad():
        lrn.actor.params.fill_(0.5)
    assert all(bool((p == 0.5).all()) for p in mu.parameters())
    assert set(mu.state_dict()) == {'0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias'}
    assert lrn.actor.hyper.tolist() == [float(F(x)) for x in (3e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0)]
    assert lrn.critics[1].hyper.tolist() == [float(F(x)) for x in (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0)]
    assert (lrn.obs_dim, lrn.action_dim, lrn.loss_kind) == (10, 1, 2)
    lrn.set_lr(actor=0.5)
    lrn.set_lr(critic=0.25)
    assert lrn.actor.hyper[0] == 0.5 and all(c.hyper[0] == 0.25 for c in lrn.critics)
    lrn.critics[0].m.fill_(1.0)
    lrn.critics[0].hyper[5:7].fill_(0.5)
    lrn.reset_optimizer()
    assert not lrn.critics[0].m.any() and lrn.critics[0].hyper[5:7].tolist() == [1.0, 1.0]


def test_refusals_on_the_host():
    """every refusal of the Python layer raises ValueError before a library call (there is no GPU here to call), and a refused
    construction leaves the modules' parameters where they were"""
    from soccer2d_amd.learn import ActorCriticLearner
    good_q = lambda: seq(11, (8,), 1)
    for mu, q, text in ((seq(10, (12,), 1, head=True), good_q(), 'multiple of 8'), (seq(10, (264,), 1, head=True), good_q(), 'multiple of 8'),
                        (seq(10, (8,) * 5, 1, head=True), good_q(), '1 to 4 hidden'), (seq(10, (8,), 1, head=True), seq(11, (400, 300), 1), 'multiple of 8'),
                        (seq(10, (8,), 9, head=True), seq(19, (8,), 1), '1 to 8'), (seq(249, (8,), 1, head=True), seq(250, (8,), 1), 'input width'),
                        (seq(10, (8,), 1, head=True), seq(12, (8,), 1), 'obs_dim [+] A'), (seq(10, (8,), 1, head=True), seq(11, (8,), 2), 'one output'),
                        (seq(10, (8,), 1, head=True, bias=False), good_q(), 'bias'), (seq(10, (8,), 1, head=True), seq(11, (8,), 1, act=nn.ELU), 'activation'),
                        (seq(10, (8,), 1, head=True).double(), good_q(), 'float32'), ('mu', good_q(), 'torch.nn.Module')):
        olds = [p.data_ptr() for m in (mu, q) if isinstance(m, nn.Module) for p in m.parameters()]
        with pytest.raises(ValueError, match=text):
            ActorCriticLearner.from_modules(mu, q, device='cpu')
        assert olds == [p.data_ptr() for m in (mu, q) if isinstance(m, nn.Module) for p in m.parameters()]
    with pytest.raises(ValueError, match='critic 2'):
        ActorCriticLearner.from_modules(seq(10, (8,), 1, head=True), good_q(), seq(12, (8,), 1), device='cpu')
    for kw, text in ((dict(loss='l1'), 'loss'), (dict(max_batch=0), 'max_batch'), (dict(betas=(0.9, 1.0)), 'betas'), (dict(actor_lr=-1.0), 'lr')):
        with pytest.raises(ValueError, match=text):
            ActorCriticLearner.from_modules(seq(10, (8,), 1, head=True), good_q(), device='cpu', **kw)
    lrn = ActorCriticLearner.from_modules(seq(10, (8,), 2, head=True), seq(12, (8,), 1), max_batch=32, device='cpu')
    before = [n.params.clone() for n in (lrn.actor,) + lrn.critics]
    B = 8
    good = dict(obs=torch.zeros(B, 10), action=torch.zeros(B, 2))
    tgt = torch.zeros(B)
    for batch, target, kw, text in (
            ({'obs': good['obs']}, tgt, {}, "'obs' and 'action'"),
            (dict(good, obs=torch.zeros(B, 9)), tgt, {}, r"batch\['obs'\]"),
            (dict(good, obs=torch.zeros(B, 10, dtype=torch.float64)), tgt, {}, r"batch\['obs'\]"),
            (dict(good, action=torch.zeros(B, 2, dtype=torch.int32)), tgt, {}, r"batch\['action'\]"),
            (dict(good, action=torch.zeros(B, 1)), tgt, {}, r"batch\['action'\]"),
            (good, torch.zeros(B + 1), {}, 'target'),
            (good, tgt, dict(weight=torch.zeros(B, 1)), 'weight'),
            (good, tgt, dict(td_abs_out=torch.zeros(B, dtype=torch.float64)), 'td_abs_out'),
            (good, tgt, dict(q_out=torch.zeros(B, 1)), 'q_out'),
            (dict(obs=torch.zeros(33, 10), action=torch.zeros(33, 2)), torch.zeros(33), {}, 'max_batch=32'),
            (good, tgt, {}, 'no CPU path')):
        with pytest.raises(ValueError, match=text):
            lrn.step_critic(batch, target, **kw)
    for batch, kw, text in (({}, {}, "'obs'"), (good, dict(action_out=torch.zeros(B, 1)), 'action_out'), (good, dict(q_out=torch.zeros(B + 1)), 'q_out'),
                            (good, {}, 'no CPU path')):
        with pytest.raises(ValueError, match=text):
            lrn.step_actor(batch, **kw)
    for call in (lambda: lrn.grad_critic(good, tgt), lambda: lrn.grad_actor(good), lambda: lrn.step(good, tgt)):
        with pytest.raises(ValueError, match='no CPU path'):
            call()
    with pytest.raises(ValueError, match='td.ActorCriticTarget'):
        lrn.update_targets(seq(10, (8,), 2))
    assert all(torch.equal(n.params, b) for n, b in zip((lrn.actor,) + lrn.critics, before))


def test_update_targets_on_the_host():
    """update_targets is torch on the flat buffers, so it runs here: lerp_ / copy_ bit for bit, the target modules follow, shapes
    and the critic count are checked"""
    from soccer2d_amd.learn import ActorCriticLearner
    from soccer2d_amd.td import ActorCriticTarget
    torch.manual_seed(4)
    mk = lambda: (seq(10, (16, 8), 2, head=True), seq(12, (16,), 1), seq(12, (8, 8), 1, act=nn.Tanh))
    mods, tmods = mk(), mk()
    lrn = ActorCriticLearner.from_modules(*mods, device='cpu')
    tgt = ActorCriticTarget.from_modules(*tmods, device='cpu')
    nets, tnets = (lrn.actor,) + lrn.critics, (tgt.mu_target,) + tgt.critics
    old = [t.params.clone() for t in tnets]
    lrn.update_targets(tgt, tau=0.005)
    for n, t, o, m in zip(nets, tnets, old, tmods):
        assert torch.equal(t.params, o.lerp(n.params, 0.005)) and not torch.equal(t.params, o)
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in m.parameters()]), t.params)
    tgt.sync()                                                               # the module round trip still works
    assert all(torch.equal(t.params, o.lerp(n.params, 0.005)) for n, t, o in zip(nets, tnets, old))
    lrn.update_targets(tgt)
    for n, t, m in zip(nets, tnets, tmods):
        assert torch.equal(t.params, n.params) and torch.equal(torch.cat([p.detach().reshape(-1) for p in m.parameters()]), n.params)
    with pytest.raises(ValueError, match='critic'):
        lrn.update_targets(ActorCriticTarget.from_modules(*mk()[:2], device='cpu'))
    with pytest.raises(ValueError, match='target critic 1 is'):
        lrn.update_targets(ActorCriticTarget.from_modules(mk()[0], seq(12, (32,), 1), mk()[2], device='cpu'))
    with pytest.raises(ValueError, match='tau'):
        lrn.update_targets(tgt, tau=1.5)
