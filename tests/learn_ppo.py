"""ctypes binding of tests/learn_ppo_ref.c (the host restatement of s2d_learn_ppo / s2d_learn_ppo_grad) and what the tests of the
fused PPO update share: models (pi, vf and log_std as views of ONE flat parameter vector), the optimiser's state with its ten hyper
words, the shape list, a rollout generator that reaches every branch of the clipped surrogate, and a torch autograd of the examples'
loss in a given dtype.  Networks are tests/td.py's Net.  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (DESIGN.md
section 4)."""
import ctypes as C
import os
import subprocess

import numpy as np

import learn as LR
import td as TD

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'learn_ppo_ref.c')
F = np.float32
BLOCK_ROWS = LR.BLOCK_ROWS
MAX_GROUPS = 256
CATEGORICAL, GAUSSIAN = 0, 1

# (D, pi hidden, A, pi activation, vf hidden, vf activation, head)
SHAPES = [
    (1, (8,), 1, 'relu', (8,), 'relu', CATEGORICAL),                     # the smallest
    (4, (8, 16), 3, 'tanh', (16, 8), 'relu', CATEGORICAL),               # mixed activations
    (13, (24, 40), 17, 'sigmoid', (24, 40), 'sigmoid', CATEGORICAL),     # tiles that are no multiples of 16
    (10, (64, 64), 16, 'tanh', (64, 64), 'tanh', CATEGORICAL),           # SB3's default
    (10, (64, 64), 1, 'relu', (64, 64), 'relu', GAUSSIAN),
    (10, (64, 64), 4, 'relu', (64, 64), 'relu', GAUSSIAN),
    (13, (24, 40), 8, 'tanh', (24, 40), 'tanh', GAUSSIAN),
    (224, (64, 64), 16, 'relu', (64, 64), 'relu', CATEGORICAL),          # 11v11: the image is in LDS
    (256, (256, 256), 64, 'relu', (256, 256), 'relu', CATEGORICAL),      # the widest: the image is in the workspace
]
REACH_BALL = SHAPES[3]
SMALL = (4, (8,), 2, 'tanh', (8,), 'tanh', CATEGORICAL)                  # the batch edges above one group of blocks


def shape_id(s):
    return f'{s[0]}-' + 'x'.join(map(str, s[1])) + f'-{s[2]}{s[3]}-' + 'x'.join(map(str, s[4])) + f'{s[5]}-' + ('cat', 'gauss')[s[6]]


class PpoCall(C.Structure):
    _fields_ = [('head', C.c_int32), ('normalize', C.c_int32), ('R', C.c_int64), ('B', C.c_int64), ('obs', C.c_void_p),
                ('action', C.c_void_p), ('logp_old', C.c_void_p), ('adv', C.c_void_p), ('ret', C.c_void_p), ('index', C.c_void_p)]


def build(outdir):
    so = os.path.join(str(outdir), 'liblearn_ppo_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V, N, Q = C.c_void_p, C.POINTER(LR.LearnNet), C.POINTER(PpoCall)
    L.ppo_param_count.restype, L.ppo_param_count.argtypes = C.c_int64, [N, N, C.c_int]
    L.ppo_blocks_per_group.restype, L.ppo_blocks_per_group.argtypes = C.c_int64, [C.c_int64]
    L.ppo_advantage_stats.restype, L.ppo_advantage_stats.argtypes = None, [Q, V, V]
    L.ppo_grad.restype, L.ppo_grad.argtypes = None, [N, N, V, Q, V, V, V, V, V, V]
    L.ppo_step.restype, L.ppo_step.argtypes = None, [N, N, V, Q, V, V, V, V, V, V, V, V, V]
    return L


_p = LR._p


class Model:
    """pi, vf (tests/td.py Nets) and log_std (head 1) as VIEWS of the flat vector [pi | vf | log_std]"""

    def __init__(self, D, hp, A, act_p, hv, act_v, head, flat):
        self.head, self.A, self.D = head, A, D
        self.P_pi, self.P_vf = TD.param_count(D, hp, A), TD.param_count(D, hv, 1)
        self.P = self.P_pi + self.P_vf + (A if head else 0)
        self.flat = np.ascontiguousarray(flat, F)
        assert self.flat.size == self.P
        self.pi = TD.Net(D, hp, A, act_p, self.flat[:self.P_pi])
        self.vf = TD.Net(D, hv, 1, act_v, self.flat[self.P_pi:self.P_pi + self.P_vf])
        self.log_std = self.flat[self.P_pi + self.P_vf:] if head else None
        assert np.shares_memory(self.pi.params, self.flat) and np.shares_memory(self.vf.params, self.flat)

    def copy(self):
        return Model(self.D, self.pi.hidden, self.A, self.pi.act, self.vf.hidden, self.vf.act, self.head, self.flat.copy())


def random_model(rs, shape, gain=1.0):
    D, hp, A, act_p, hv, act_v, head = shape
    pi, vf = TD.random_net(rs, D, hp, A, act_p, gain), TD.random_net(rs, D, hv, 1, act_v, gain)
    ls = [rs.uniform(-0.7, 0.3, A).astype(F)] if head else []
    return Model(D, hp, A, act_p, hv, act_v, head, np.concatenate([pi.params, vf.params] + ls))


class State:
    """the optimiser's state of the spec: m, v, hyper = (lr, beta1, beta2, eps, max_grad_norm, beta1^t, beta2^t, clip_range, vf_coef,
    ent_coef)"""

    def __init__(self, P, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5, clip_range=0.2, vf_coef=0.5, ent_coef=0.0):
        self.m, self.v = np.zeros(P, F), np.zeros(P, F)
        self.hyper = np.array([lr, betas[0], betas[1], eps, max_grad_norm, 1.0, 1.0, clip_range, vf_coef, ent_coef], F)


def _call(model, ro, index, B, normalize):
    """(PpoCall, the arrays it points to, B)"""
    R = ro['obs'].shape[0]
    arrs = [np.ascontiguousarray(ro['obs'], F), np.ascontiguousarray(ro['action'], F if model.head else np.int32),
            np.ascontiguousarray(ro['logp'], F), np.ascontiguousarray(ro['advantage'], F), np.ascontiguousarray(ro['return'], F),
            np.ascontiguousarray(index, np.int32) if index is not None else None]
    assert arrs[0].shape == (R, model.D) and arrs[1].shape == ((R, model.A) if model.head else (R,)) and all(a.shape == (R,) for a in arrs[2:5])
    if B is None:
        B = arrs[5].size if index is not None else R
    assert index is None and B <= R or index is not None and arrs[5].shape == (B,)
    return PpoCall(model.head, int(normalize), R, B, *(_p(a) for a in arrs)), arrs, B


def _run(L, fn, model, state, ro, index, B, normalize):
    call, keep, B = _call(model, ro, index, B, normalize)
    g, stats, logp, value = np.zeros(model.P, F), np.zeros(8, F), np.zeros(B, F), np.zeros(B, F)
    err = np.zeros(1, np.int32)
    cp, cv = LR.c_net(model.pi), LR.c_net(model.vf)
    if fn == 'grad':
        L.ppo_grad(C.byref(cp), C.byref(cv), _p(model.log_std), C.byref(call), _p(state.hyper), _p(g), _p(stats), _p(logp), _p(value), _p(err))
    else:
        L.ppo_step(C.byref(cp), C.byref(cv), _p(model.log_std), C.byref(call), _p(model.flat), _p(state.m), _p(state.v), _p(g),
                   _p(state.hyper), _p(stats), _p(logp), _p(value), _p(err))
    del keep
    return dict(grad=g, stats=stats, logp=logp, value=value, error=int(err[0]))


def grad(L, model, state, ro, index=None, B=None, normalize=True):
    """dict(grad [P], stats [8], logp [B], value [B], error); only state.hyper is read"""
    return _run(L, 'grad', model, state, ro, index, B, normalize)


def step(L, model, state, ro, index=None, B=None, normalize=True):
    """one s2d_learn_ppo on model.flat and state (both in place); returns grad()'s dict"""
    return _run(L, 'step', model, state, ro, index, B, normalize)


def advantage_stats(L, model, ro, index=None, B=None):
    call, keep, B = _call(model, ro, index, B, True)
    mean, std = np.zeros(1, F), np.zeros(1, F)
    L.ppo_advantage_stats(C.byref(call), _p(mean), _p(std))
    return mean[0], std[0]


def random_rollout(rs, L, model, R, spread=0.25):
    """R rows: obs U(-1, 1); actions uniform (categorical) or the mean + sigma N(0, 1); logp_old = the model's own logp (the
    restatement's) + N(0, spread): with spread 0.25 and a clip range of 0.2 about four rows in ten leave [1 - c, 1 + c], on both sides;
    advantages N(0.3, 1): both signs, so every branch of the clipped surrogate is reached; returns = the model's value + N(0.5, 0.7)
    (off zero: see tests/learn_ac.py on the conditioning of the output bias's sum)."""
    obs = rs.uniform(-1, 1, (R, model.D)).astype(F)
    if model.head:
        mu = TD.forward64(model.pi, obs)
        action = (mu + np.exp(model.log_std.astype(np.float64)) * rs.normal(0, 1, (R, model.A))).astype(F)
    else:
        action = rs.randint(0, model.A, R).astype(np.int32)
    ro = dict(obs=obs, action=action, logp=np.zeros(R, F), advantage=rs.normal(0.3, 1.0, R).astype(F), **{'return': np.zeros(R, F)})
    own = grad(L, model, State(model.P), ro, normalize=False)
    ro['logp'] = (own['logp'] + rs.normal(0, spread, R)).astype(F)
    ro['return'] = (own['value'] + rs.normal(0.5, 0.7, R)).astype(F)
    return ro


def regimes(L, model, state, ro, index=None, B=None, normalize=True):
    """what the restatement's output says of the rows of a call: dict(clip_fraction, above_clipped, below_clipped, outside_passing,
    adv_pos, adv_neg) as counts (clip_fraction the statistic itself)"""
    out = grad(L, model, state, ro, index, B, normalize)
    rows = np.arange(out['logp'].size) if index is None else np.asarray(index)
    adv = ro['advantage'][rows].astype(np.float64)
    if normalize and rows.size > 1:
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    r = np.exp(out['logp'].astype(np.float64) - ro['logp'][rows])
    c = float(state.hyper[7])
    hi, lo = r > 1 + c, r < 1 - c
    return dict(clip_fraction=float(out['stats'][7]), above_clipped=int((hi & (adv > 0)).sum()), below_clipped=int((lo & (adv < 0)).sum()),
                outside_passing=int(((hi & (adv < 0)) | (lo & (adv > 0))).sum()), adv_pos=int((adv > 0).sum()), adv_neg=int((adv < 0).sum()))


def reaches_every_branch(g):
    return (0.05 < g['clip_fraction'] < 0.95 and g['above_clipped'] > 0 and g['below_clipped'] > 0 and g['outside_passing'] > 0
            and g['adv_pos'] > 0 and g['adv_neg'] > 0)


def torch_grad(model, state, ro, index=None, normalize=True, dtype=None):
    """(flat gradient [pi | vf | log_std] as float64 NumPy, dict of the loss's parts) of the examples' loss by torch autograd in
    `dtype`: Categorical / Normal log_prob and entropy, per-minibatch advantage normalisation, min / clamp, F.mse_loss"""
    import torch
    dtype = dtype or torch.float64
    pi, vf = LR.torch_module(model.pi, dtype), LR.torch_module(model.vf, dtype)
    params = list(pi.parameters()) + list(vf.parameters())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    i = t(np.asarray(index)).long() if index is not None else torch.arange(ro['obs'].shape[0])
    obs, logp_old, adv, ret = (t(ro[k]).to(dtype)[i] for k in ('obs', 'logp', 'advantage', 'return'))
    clip, vf_coef, ent_coef = (float(x) for x in state.hyper[7:10])
    y = pi(obs)
    if model.head:
        log_std = t(model.log_std.copy()).to(dtype).requires_grad_(True)
        params.append(log_std)
        d = torch.distributions.Independent(torch.distributions.Normal(y, log_std.exp().expand_as(y)), 1)
        logp = d.log_prob(t(ro['action']).to(dtype)[i])
    else:
        d = torch.distributions.Categorical(logits=y)
        logp = d.log_prob(t(ro['action']).long()[i])
    if normalize and i.numel() > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = (logp - logp_old).exp()
    pg_rows = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv)
    pg = pg_rows.mean()
    value = vf(obs).squeeze(-1)
    v_loss = torch.nn.functional.mse_loss(value, ret)
    ent_rows = d.entropy()
    ent = ent_rows.mean()
    loss = pg + vf_coef * v_loss - ent_coef * ent
    loss.backward()
    flat = np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().numpy().reshape(-1) for p in params])
    kl_rows = (ratio - 1) - (logp - logp_old)
    mean_abs = lambda t: float(t.detach().abs().double().mean())
    return flat, dict(loss=float(loss.detach()), pg=float(pg.detach()), v_loss=float(v_loss.detach()), entropy=float(ent.detach()),
                      approx_kl=float(kl_rows.mean().detach()), clip_fraction=float(((ratio - 1).abs() > clip).double().mean()),
                      clipped_rows=int(((ratio - 1).abs() > clip).sum()),
                      # the mean size of a row's term in each mean: what a summation-order bound scales with
                      row_abs=dict(pg=mean_abs(pg_rows), v_loss=mean_abs((value - ret) ** 2), entropy=mean_abs(ent_rows), approx_kl=mean_abs(kl_rows)))
