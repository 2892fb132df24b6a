"""CPU checks of the fused PPO update's host side (s2d_learn_ppo / s2d_learn_ppo_grad, soccer2d_amd.learn.PPOLearner): the ABI
additions, the workspace arithmetic, and the host restatement tests/learn_ppo_ref.c -- its categorical logp against policy_ref.c's
head bitwise, its gradient and loss against float64 torch autograd of the examples' loss, hand-computed rows of the clipped
surrogate, Adam and the clip over the combined buffer, the batch generator's regimes -- and the argument checks of the class that
raise before any library call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import learn as LR
import learn_ppo as PP
import policy_ref as PR
import td as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return PP.build(tmp_path_factory.mktemp('learn_ppo_ref'))


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_additions(tmp_path):
    """the ABI version stays 4, S2DLearnNet and S2DLearnState keep their sizes, the new structs have the mirror's, and the header
    declares the three functions"""
    from soccer2d_amd import _capi, learn
    prog = tmp_path / 'learn_ppo_abi.c'
    prog.write_text('#include <stdio.h>\n#include "s2d.h"\nint main(){printf("%d %d %d %d %zu %zu %zu %zu %zu", S2D_ABI_VERSION, '
                    'S2D_LEARN_PPO_MAX_GROUPS, S2D_LEARN_PPO_CATEGORICAL, S2D_LEARN_PPO_GAUSSIAN, sizeof(S2DLearnNet), sizeof(S2DLearnState), '
                    'sizeof(S2DLearnPPO), sizeof(S2DLearnPPOBatch), sizeof &s2d_learn_ppo + sizeof &s2d_learn_ppo_grad + '
                    'sizeof &s2d_learn_ppo_workspace_bytes);return 0;}\n')
    exe = tmp_path / 'learn_ppo_abi'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [4, PP.MAX_GROUPS, PP.CATEGORICAL, PP.GAUSSIAN, C.sizeof(_capi.S2DLearnNet), C.sizeof(_capi.S2DLearnState),
                   C.sizeof(_capi.S2DLearnPPO), C.sizeof(_capi.S2DLearnPPOBatch), 3 * C.sizeof(C.c_void_p)]
    assert learn.PPO_MAX_GROUPS == PP.MAX_GROUPS and learn.PPO_HEADS == ('categorical', 'gaussian')


def _shape(n_in, hidden, n_out, act=0):
    from soccer2d_amd import _capi
    s = _capi.S2DLearnNet()
    s.n_in, s.n_hidden, s.n_out, s.activation = n_in, len(hidden), n_out, act
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    return s


def test_symbols_exported_and_workspace_arithmetic(L):
    """the built library exports and binds the three symbols; s2d_learn_ppo_workspace_bytes (host only) agrees with the Python
    arithmetic on the grid, is 0 off it, and does not grow with the minibatch beyond the 256 groups and the O(B) row scratch"""
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    from soccer2d_amd.learn import learn_param_count, learn_ppo_workspace_bytes
    lib = _capi.load_library()
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    for name, nargs in (('s2d_learn_ppo', 3), ('s2d_learn_ppo_grad', 3), ('s2d_learn_ppo_workspace_bytes', 4)):
        assert hasattr(lib, name) and len(protos[name][2]) == nargs, name

    def ws(D, hp, A, hv, head, B):
        return lib.s2d_learn_ppo_workspace_bytes(C.byref(_shape(D, hp, A)), C.byref(_shape(D, hv, 1)), head, B)
    for D, hp, A, _, hv, _, head in PP.SHAPES + [PP.SMALL, (256, (256,) * 4, 8, 'relu', (256,) * 4, 'relu', 1)]:
        P = learn_param_count(D, hp, A) + learn_param_count(D, hv, 1) + (A if head else 0)
        last = 0
        for B in (1, 63, 64, 65, 4096, 16384, 16385, 49217, 180224, 2 ** 31 - 1):
            got = ws(D, hp, A, hv, head, B)
            assert got == learn_ppo_workspace_bytes(D, hp, A, hv, head, B) and got >= last, (D, hp, A, hv, head, B)
            last = got
        pitch = (D + 3) // 4 * 4 + sum(hp) + A + sum(hv) + 1 + (A if head else 0) + 1
        assert ws(D, hp, A, hv, head, 180224) <= 4 * (256 * (P + 8 + 64 * pitch) + P // 256 + 180224 // 64 + 6 * 64)
    # the 11v11 minibatch of the issue: far below the 430 MB that block partials would take
    assert ws(224, (64, 64), 16, (64, 64), 0, 180224) < 45e6
    # 64 rows of the 11v11 pair fit the LDS, 64 rows of the widest pair do not: its images are in the workspace
    P = lambda D, h, A: learn_param_count(D, h, A) + learn_param_count(D, h, 1)
    assert ws(224, (64, 64), 16, (64, 64), 0, 64) < 4 * (P(224, (64, 64), 16) + 64 * 8)
    assert ws(256, (256, 256), 64, (256, 256), 0, 64) > 4 * (P(256, (256, 256), 64) + 64 * 1345)
    for args in (((10, (64,), 0), (10, (64,), 1), 0), ((10, (64,), 65), (10, (64,), 1), 0), ((10, (64,), 9), (10, (64,), 1), 1),
                 ((10, (64,), 4), (11, (64,), 1), 0), ((10, (64,), 4), (10, (64,), 2), 0), ((10, (12,), 4), (10, (64,), 1), 0),
                 ((10, (64,), 4), (10, (64,) * 5, 1), 0), ((257, (64,), 4), (257, (64,), 1), 0), ((10, (64,), 4), (10, (64,), 1), 2),
                 ((10, (64,), 4), (10, (64,), 1), -1)):
        assert lib.s2d_learn_ppo_workspace_bytes(C.byref(_shape(*args[0])), C.byref(_shape(*args[1])), args[2], 64) == 0, args
    assert lib.s2d_learn_ppo_workspace_bytes(C.byref(_shape(10, (64,), 4, act=3)), C.byref(_shape(10, (64,), 1)), 0, 64) == 0
    good = (_shape(10, (64,), 4), _shape(10, (64,), 1))
    assert lib.s2d_learn_ppo_workspace_bytes(None, C.byref(good[1]), 0, 64) == 0 == lib.s2d_learn_ppo_workspace_bytes(C.byref(good[0]), None, 0, 64)
    for B in (0, -1, 2 ** 31):
        assert lib.s2d_learn_ppo_workspace_bytes(C.byref(good[0]), C.byref(good[1]), 1, B) == 0
    assert lib.s2d_learn_ppo_workspace_bytes(C.byref(good[0]), C.byref(good[1]), 1, 1) > 0
    # the groups are a function of B alone
    assert [L.ppo_blocks_per_group(B) for B in (1, 64, 16384, 16385, 32768, 49217, 180224)] == [1, 1, 1, 2, 2, 4, 11]


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_categorical_logp_equals_policy_ref(L, tmp_path, act):
    """out_logp and the logits' path are policy_ref.c's: for the actions its categorical head draws from its own forward pass of the
    same parameters, the restatement's logp has the head's bits, edge rows included -- so the ratio at collection is exactly 1"""
    P = PR.build(tmp_path)
    rs = np.random.RandomState(5)
    model = PP.random_model(rs, (10, (64, 64), 16, act, (64, 64), act, 0), gain=2.0)
    R = 300
    obs = rs.uniform(-1, 1, (R, 10)).astype(F)
    obs[0] = 0.0
    obs[1] = -0.0
    obs[2] = 50.0
    y = PR.forward(P, obs, model.pi.params, 64, 64, 16, act == 'tanh')
    action, logp = PR.categorical(P, y, rs.randint(0, 2 ** 32, R, dtype=np.uint64).astype(np.uint32))
    assert len(set(action.tolist())) > 8
    ro = dict(obs=obs, action=action, logp=logp, advantage=rs.normal(0, 1, R).astype(F), **{'return': np.zeros(R, F)})
    got = PP.grad(L, model, PP.State(model.P), ro)
    assert np.array_equal(TD.bits(got['logp']), TD.bits(logp))
    assert got['stats'][6] == 0 and got['stats'][7] == 0 and got['error'] == 0


CASES64 = [(s, n, e) for s in PP.SHAPES[1:8] for n in (True, False) for e in (0.0, 0.01)]


@pytest.mark.parametrize('shape, normalize, ent_coef', CASES64, ids=lambda v: PP.shape_id(v) if isinstance(v, tuple) else str(v))
def test_gradient_against_float64_autograd(L, shape, normalize, ent_coef):
    """the restated gradient over [pi | vf | log_std] against float64 torch autograd of the examples' loss: at most 4 x the largest
    error of torch's own fp32 autograd on the same inputs, the bound computed here; the loss's parts likewise.  B = 150 rows named by
    a permutation slice of 400: three blocks, the last partial."""
    rs = np.random.RandomState(11)
    model = PP.random_model(rs, shape)
    ro = PP.random_rollout(rs, L, model, 400)
    index = rs.permutation(400)[:150].astype(np.int32)
    st = PP.State(model.P, max_grad_norm=0.0, ent_coef=ent_coef)
    assert PP.reaches_every_branch(PP.regimes(L, model, st, ro, index, normalize=normalize))
    g64, l64 = PP.torch_grad(model, st, ro, index, normalize, torch.float64)
    g32, l32 = PP.torch_grad(model, st, ro, index, normalize, torch.float32)
    got = PP.grad(L, model, st, ro, index, normalize=normalize)
    err_torch, err_ref = np.abs(g32 - g64).max(), np.abs(got['grad'].astype(np.float64) - g64).max()
    print(f'grad error vs float64: torch fp32 {err_torch:.3e}, learn_ppo_ref {err_ref:.3e}; |g|max {np.abs(g64).max():.3e}')
    assert err_torch > 0 and err_ref <= 4 * err_torch
    # The statistics are means of B row terms summed sequentially in fp32, where torch sums pairwise: to the project's criterion (4 x
    # torch's fp32 error, at least half a unit of the value) the worst case of the spec's order is added, (B - 1) u sum|t| / B =
    # (B - 1) u mean|t| with u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), the mean taken over the
    # float64 row terms.  The loss is pg + vf_coef v_loss - ent_coef entropy, so its allowance is the parts' in that combination.
    ra, u = l64['row_abs'], 149 * 2.0 ** -24
    order = dict(ra, loss=ra['pg'] + float(st.hyper[8]) * ra['v_loss'] + float(st.hyper[9]) * ra['entropy'])
    for k, name in ((0, 'loss'), (3, 'pg'), (4, 'v_loss'), (5, 'entropy'), (6, 'approx_kl')):
        e_t, e_r = abs(l32[name] - l64[name]), abs(float(got['stats'][k]) - l64[name])
        bound = 4 * max(e_t, np.spacing(F(abs(l64[name]))) / 2) + u * order[name]
        print(f'{name}: float64 {l64[name]:.6f}, torch fp32 error {e_t:.3e}, learn_ppo_ref error {e_r:.3e}, bound {bound:.3e}')
        assert e_r <= bound
    # clip_fraction is a count: exact, as torch's
    assert l32['clipped_rows'] == l64['clipped_rows'] and got['stats'][7] == F(l64['clipped_rows']) / F(150)
    norm64 = np.sqrt((g64 ** 2).sum())
    assert abs(float(got['stats'][1]) - norm64) <= 4 * max(err_torch, np.spacing(F(norm64))) and float(got['stats'][2]) == 1.0


def test_advantage_prepass(L):
    """mean and unbiased standard deviation over the rows the index names, repeated rows counted as often as named"""
    rs = np.random.RandomState(2)
    model = PP.random_model(rs, PP.SMALL)
    ro = PP.random_rollout(rs, L, model, 500)
    index = rs.randint(0, 500, 333).astype(np.int32)
    mean, std = PP.advantage_stats(L, model, ro, index)
    a = ro['advantage'][index].astype(np.float64)
    assert abs(mean - a.mean()) < 1e-6 and abs(std - a.std(ddof=1)) < 1e-6


def test_hand_computed_rows(L):
    """A policy net of zeros: logits (0, 0), p = (1/2, 1/2), so with action 0 the output-bias gradient is g (1/2, -1/2) with g the
    derivative of the row's policy loss in logp.  One row per call (B = 1: no normalisation), c = 0.2:
      r = e^0.5 above 1 + c with A^ = 2: the clip is active, g = +0 and the whole policy gradient is +0, bit for bit
      the same r with A^ = -2: min takes the unclipped term, g = -(A^ r) = 2 r
      r exactly 1 (logp_old = logp) with c = 0, so r == 1 + c: the boundary passes, g = -A^ = -2, db = (-1, 1) exactly
      r exactly 1.25 with c = 0.25: the same, g = -2.5; one ulp above it the clip is active"""
    model = PP.Model(1, (8,), 2, 'tanh', (8,), 'tanh', 0, np.zeros(PP.TD.param_count(1, (8,), 2) + PP.TD.param_count(1, (8,), 1), F))
    model.vf.params[-1] = 0.25
    base = dict(obs=np.ones((1, 1), F), action=np.zeros(1, np.int32), logp=np.zeros(1, F), advantage=np.full(1, 2, F), **{'return': np.ones(1, F)})
    own = PP.grad(L, model, PP.State(model.P), base)['logp']
    assert abs(own[0] + np.log(2)) < 1e-7
    ob = slice(model.P_pi - 2, model.P_pi)                                  # pi's output biases

    def run(logp_old, adv, clip):
        ro = dict(base, logp=np.array([logp_old], F), advantage=np.full(1, adv, F))
        return PP.grad(L, model, PP.State(model.P, max_grad_norm=0.0, clip_range=clip), ro)
    got = run(own[0] - 0.5, 2.0, 0.2)
    assert (TD.bits(got['grad'][:model.P_pi]) == 0).all() and got['stats'][7] == 1
    assert abs(got['stats'][3] + 2 * 1.2) < 1e-6                            # the clipped surrogate's value: -(1 + c) A^
    assert np.allclose(got['grad'][-1], 0.5 * 2 * (0.25 - 1.0), rtol=1e-6)  # vf_coef 2 e into the value net's output bias
    got = run(own[0] - 0.5, -2.0, 0.2)
    r = np.exp(0.5)
    assert np.allclose(got['grad'][ob], [2 * r * 0.5, -2 * r * 0.5], rtol=1e-6) and got['stats'][7] == 1
    assert abs(got['stats'][3] - 2 * r) < 1e-5
    got = run(own[0], 2.0, 0.0)
    assert got['grad'][ob].tolist() == [-1.0, 1.0] and got['stats'][7] == 0 and got['stats'][6] == 0 and got['stats'][3] == -2.0
    # just above the boundary the clip takes over
    got = run(np.nextafter(own[0], F(-1), dtype=F) - F(1e-6), 2.0, 0.0)
    assert (TD.bits(got['grad'][:model.P_pi]) == 0).all() and got['stats'][7] == 1
    # the same at c = 0.25: among the logp_old next to logp - ln 1.25, those whose ratio (read back as the unclipped surrogate at
    # A^ = 1 under a clip range that never acts) is exactly 1.25 pass with g = -2.5, db = (-1.25, 1.25); the next ratio up is clipped
    near, seen = F(own[0] - np.log(1.25)), {}
    for k in range(-40, 41):
        old = near
        for _ in range(abs(k)):
            old = np.nextafter(old, F(np.sign(k) * 10), dtype=F)
        seen[float(old)] = float(-run(old, 1.0, 10.0)['stats'][3])
    exact = [o for o, r in seen.items() if r == 1.25]
    above = [o for o, r in seen.items() if r == float(np.nextafter(F(1.25), F(2), dtype=F))]
    assert exact and above
    for o in exact:
        got = run(o, 2.0, 0.25)
        assert got['grad'][ob].tolist() == [-1.25, 1.25] and got['stats'][7] == 0 and got['stats'][3] == -2.5
    for o in above:
        got = run(o, 2.0, 0.25)
        assert (TD.bits(got['grad'][:model.P_pi]) == 0).all() and got['stats'][7] == 1 and got['stats'][3] == -2.5


@pytest.mark.parametrize('head', [0, 1])
def test_adam_and_clip_over_the_combined_buffer(L, head):
    """three steps on one minibatch against torch: ONE clip_grad_norm_ over pi, vf and log_std and ONE Adam over all of them in
    float64; the restated norm is the norm of the whole buffer, the scale its clip, and m, v, the parameters follow"""
    rs = np.random.RandomState(4)
    shape = (10, (16, 8), 4, 'tanh', (8, 16), 'relu', head)
    model = PP.random_model(rs, shape)
    ro = PP.random_rollout(rs, L, model, 200)
    st = PP.State(model.P, lr=1e-2, max_grad_norm=0.05, ent_coef=0.01)
    ref = model.copy()
    m64, v64 = np.zeros(model.P), np.zeros(model.P)
    for t in range(1, 4):
        g64, _ = PP.torch_grad(ref, st, ro, None, True, torch.float64)
        norm = np.sqrt((g64 ** 2).sum())
        scale = min(1.0, 0.05 / (norm + 1e-6))
        got = PP.step(L, model, st, ro)
        assert abs(got['stats'][1] - norm) < 1e-5 * norm and abs(got['stats'][2] - scale) < 1e-5 * scale and scale < 1
        g = g64 * scale
        m64, v64 = 0.9 * m64 + 0.1 * g, 0.999 * v64 + 0.001 * g * g
        upd = 1e-2 / (1 - 0.9 ** t) * m64 / (np.sqrt(v64) / np.sqrt(1 - 0.999 ** t) + 1e-5)
        ref.flat[:] = (ref.flat.astype(np.float64) - upd).astype(F)
        assert np.abs(model.flat - ref.flat).max() < 2e-5 and np.abs(st.m - m64).max() < 1e-6
        ref.flat[:] = model.flat                                             # the next step starts from the same point
    assert np.allclose(st.hyper[5:7], [0.9 ** 3, 0.999 ** 3], rtol=1e-6) and (st.hyper[7:] == np.array([0.2, 0.5, 0.01], F)).all()
    if head:
        assert (st.m[-4:] != 0).all()                                       # log_std is stepped with the rest


def test_dropped_rows(L):
    """An index at R drops its row (error bit 2), a categorical action outside [0, A) its own (bit 1).  The rest of the call is
    bitwise what it is with that row's deltas at zero, shown against a row whose deltas are zero by construction: rollout row 300
    has advantage 0 (normalisation and entropy bonus off: g = -0) and a return equal to the value net's own output (e = 0).  With the
    minibatch's row 70 pointed at it instead of past the end, or in the place of the row with the bad action, the gradient, its norm,
    the policy and value losses and every other row's outputs have the same bits; entropy, approx_kl and clip_fraction differ, since
    the zero-delta row still has a share in them and the dropped row has none."""
    rs = np.random.RandomState(6)
    model = PP.random_model(rs, PP.SMALL)
    ro = PP.random_rollout(rs, L, model, 301)
    st = PP.State(model.P, ent_coef=0.0)
    index = rs.permutation(300)[:200].astype(np.int32)
    ro['advantage'][300] = 0.0
    ro['return'][300] = PP.grad(L, model, st, ro, np.array([300], np.int32), normalize=False)['value'][0]
    keep = np.ones(200, bool)
    keep[70] = False

    def same_but_for_the_row(dropped, zeroed):
        for k in ('grad',):
            assert np.array_equal(TD.bits(dropped[k]), TD.bits(zeroed[k])), k
        assert np.array_equal(TD.bits(dropped['stats'][[1, 2, 3, 4]]), TD.bits(zeroed['stats'][[1, 2, 3, 4]]))
        for k in ('logp', 'value'):
            assert np.array_equal(TD.bits(dropped[k][keep]), TD.bits(zeroed[k][keep])), k
        assert dropped['stats'][5] < zeroed['stats'][5]                      # the dropped row has no share in the entropy
    bad, alt = index.copy(), index.copy()
    bad[70], alt[70] = 301, 300
    got, zero = PP.grad(L, model, st, ro, bad, normalize=False), PP.grad(L, model, st, ro, alt, normalize=False)
    assert got['error'] == 2 and zero['error'] == 0 and got['logp'][70] == 0 and got['value'][70] == 0 and zero['value'][70] == ro['return'][300]
    same_but_for_the_row(got, zero)
    # a bad action on the zero-delta row itself: dropped for its action, its input still loaded, nothing else moves
    ro2 = dict(ro, action=ro['action'].copy())
    ro2['action'][300] = 2
    got2 = PP.grad(L, model, st, ro2, alt, normalize=False)
    assert got2['error'] == 1 and got2['logp'][70] == 0 and got2['value'][70] == 0
    same_but_for_the_row(got2, zero)
    full = PP.grad(L, model, st, ro, index, normalize=False)
    assert full['error'] == 0 and not np.array_equal(full['grad'], got['grad'])


def test_generator_reaches_every_branch_for_the_seeds_the_gpu_tests_use(L):
    import test_gpu_learn_ppo as G
    for shape, B, seed in G.regime_inputs():
        rs = np.random.RandomState(seed)
        model = PP.random_model(rs, shape)
        ro = PP.random_rollout(rs, L, model, B + 40)
        index = rs.permutation(B + 40)[:B].astype(np.int32)
        for normalize in (True, False):
            g = PP.regimes(L, model, PP.State(model.P), ro, index, normalize=normalize)
            assert PP.reaches_every_branch(g), (shape, B, seed, g)


# ------------------------------------------------------------------------------------------------------------------ the class
def mlp(n_in, hidden, n_out, act=nn.Tanh):
    layers, win = [], n_in
    for w in hidden:
        layers += [nn.Linear(win, w), act()]
        win = w
    return nn.Sequential(*layers, nn.Linear(win, n_out))


def test_parameters_and_log_std_are_views_of_the_flat_buffer():
    from soccer2d_amd.learn import PPOLearner
    torch.manual_seed(0)
    pi, vf, log_std = mlp(10, (64, 64), 4), mlp(10, (32, 16), 1, nn.ReLU), nn.Parameter(torch.full((4,), -0.5))
    want = torch.cat([p.detach().reshape(-1).clone() for p in list(pi.parameters()) + list(vf.parameters())] + [log_std.detach().clone()])
    lrn = PPOLearner.from_modules(pi, vf, log_std=log_std, max_batch=256)
    assert lrn.head == 1 and torch.equal(lrn.params, want) and lrn.params.numel() == lrn.P_pi + lrn.P_vf + 4
    lo, hi = lrn.params.data_ptr(), lrn.params.data_ptr() + 4 * lrn.params.numel()
    assert all(lo <= p.data_ptr() < hi for p in list(pi.parameters()) + list(vf.parameters()) + [log_std])
    with torch.no_grad():
        lrn.params.add_(1.0)
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in list(pi.parameters()) + list(vf.parameters())] + [log_std.detach()]), want + 1)
    assert set(pi.state_dict()) == {'0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias'} and vf(torch.zeros(3, 10)).shape == (3, 1)
    assert lrn.hyper.tolist() == [float(F(x)) for x in (3e-4, 0.9, 0.999, 1e-5, 0.5, 1.0, 1.0, 0.2, 0.5, 0.0)]
    lrn.set_lr(0.25), lrn.set_clip_range(0.125), lrn.set_coefs(vf_coef=1.0, ent_coef=0.5)
    lrn.m.fill_(1.0), lrn.hyper[5:7].fill_(0.5), lrn.reset_optimizer()
    assert lrn.hyper.tolist() == [0.25, float(F(0.9)), float(F(0.999)), float(F(1e-5)), 0.5, 1.0, 1.0, 0.125, 1.0, 0.5] and not lrn.m.any()
    cat = PPOLearner.from_modules(mlp(10, (64, 64), 16), mlp(10, (64, 64), 1))
    assert cat.head == 0 and cat.log_std is None and cat.params.numel() == cat.P_pi + cat.P_vf


def test_host_refusals():
    from soccer2d_amd.learn import PPOLearner
    pi, vf = mlp(10, (64, 64), 16), mlp(10, (64, 64), 1)
    for args, kw, text in (((mlp(10, (400, 300), 16), vf), {}, r'multiple of 8 in \[8, 256\]'), ((pi, mlp(11, (64,), 1)), {}, 'value network'),
                           ((pi, mlp(10, (64,), 2)), {}, 'value network'), ((mlp(10, (64,), 65), vf), {}, 'categorical head'),
                           ((pi, vf), dict(log_std=nn.Parameter(torch.zeros(16))), 'Gaussian head'),
                           ((mlp(10, (64,), 4), vf), dict(log_std=torch.zeros(4)), 'log_std'),
                           ((mlp(10, (64,), 4), vf), dict(log_std=nn.Parameter(torch.zeros(3))), 'log_std'),
                           ((pi, vf), dict(max_batch=0), 'max_batch'), ((pi, vf), dict(lr=-1.0), 'lr'), ((pi, vf), dict(clip_range=-0.1), 'clip_range'),
                           ((mlp(300, (64,), 4), mlp(300, (64,), 1)), {}, 'input width'), ((pi, 'vf'), {}, 'torch.nn.Module')):
        with pytest.raises(ValueError, match=text):
            PPOLearner.from_modules(*args, **kw)
    lrn = PPOLearner.from_modules(pi, vf, max_batch=64)
    R = 100
    ro = {'obs': torch.zeros(R, 10), 'action': torch.zeros(R, dtype=torch.int32), 'logp': torch.zeros(R), 'advantage': torch.zeros(R),
          'return': torch.zeros(R)}
    idx = torch.arange(64, dtype=torch.int32)
    for r_, i_, kw, text in (({k: v for k, v in ro.items() if k != 'logp'}, idx, {}, "'logp'"), (dict(ro, obs=torch.zeros(R, 11)), idx, {}, r"rollout\['obs'\]"),
                             (dict(ro, action=ro['action'].long()), idx, {}, r"rollout\['action'\]"), (dict(ro, advantage=torch.zeros(R - 1)), idx, {}, 'advantage'),
                             (dict(ro, **{'return': torch.zeros(R, dtype=torch.float64)}), idx, {}, 'return'), (ro, idx.long(), {}, 'index'),
                             (ro, torch.arange(65, dtype=torch.int32), {}, 'max_batch=64'), (ro, None, {}, 'max_batch=64'),
                             (ro, idx, dict(logp_out=torch.zeros(63)), 'logp_out'), (ro, idx, dict(value_out=torch.zeros(128)[::2]), 'value_out'),
                             (ro, torch.zeros(0, dtype=torch.int32), {}, 'index'), ([1], idx, {}, 'dict')):
        with pytest.raises(ValueError, match=text):
            lrn.step(r_, i_, **kw)
    with pytest.raises(ValueError, match='no CPU path'):
        lrn.grad(ro, idx)
