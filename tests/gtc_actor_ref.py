"""ctypes binding of tests/gtc_actor_ref.c (the host restatement of the GoToCenter fused actors: the 4-input network, Philox with
the GoToCenter keys, the threshold and both heads), the float64 forward with its running error bound for input width 4
(tests/wide_f64.py fixes the width at 10), and the closed loop of the restatement through the GoToCenter oracle that the CPU and
the GPU tests share.  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'gtc_actor_ref.c')
ACT = {'relu': 0, 'tanh': 1, 'sigmoid': 2}
F = np.float32
IN = 4
SIGMOID_ERR = 1.0e-7          # tests/wide_ref.py: measured 8.93e-8


def build(outdir):
    so = os.path.join(str(outdir), 'libgtc_actor_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    vp, i64, u64 = C.c_void_p, C.c_int64, C.c_uint64
    for name, res, args in (
            ('gtc_forward', None, [i64, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp]),
            ('gtc_threshold', u64, [C.c_float]),
            ('gtc_explore_words', None, [i64, u64, u64, vp, vp, vp]),
            ('gtc_gauss', None, [i64, u64, u64, vp, vp, vp]),
            ('gtc_argmax', None, [i64, vp, C.c_int, vp]),
            ('gtc_q_actions', None, [i64, vp, C.c_int, C.c_float, u64, u64, vp, vp, vp, vp]),
            ('gtc_actor_actions', None, [i64, vp, C.c_int, C.c_float, C.c_int, vp, u64, u64, vp, vp, vp, vp])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=F)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def param_count(hidden, na):
    n, win = 0, IN
    for w in tuple(hidden) + (na,):
        n += w * win + w
        win = w
    return n


def forward(L, x, params, hidden, na, act):
    """y[n][na] of observations x[n][4]; act 'relu' | 'tanh' | 'sigmoid'"""
    x, params = _f32(x), _f32(params)
    assert x.ndim == 2 and x.shape[1] == IN and params.size == param_count(hidden, na), (x.shape, params.size)
    h = _i32(hidden)
    y = np.zeros((x.shape[0], na), dtype=F)
    L.gtc_forward(x.shape[0], x.ctypes.data, params.ctypes.data, len(h), h.ctypes.data, na, ACT[act], y.ctypes.data)
    return y


def argmax(L, y):
    y = _f32(y)
    out = np.zeros(y.shape[0], dtype=np.int32)
    L.gtc_argmax(y.shape[0], y.ctypes.data, y.shape[1], out.ctypes.data)
    return out


def explore_words(L, seed, gid0, episode, step):
    episode, step = _i32(episode), _i32(step)
    out = np.zeros(episode.size, dtype=np.uint32)
    L.gtc_explore_words(episode.size, int(seed), int(gid0), episode.ctypes.data, step.ctypes.data, out.ctypes.data)
    return out


def gauss(L, seed, gid0, episode, step):
    episode, step = _i32(episode), _i32(step)
    z = np.zeros((episode.size, 4), dtype=F)
    L.gtc_gauss(episode.size, int(seed), int(gid0), episode.ctypes.data, step.ctypes.data, z.ctypes.data)
    return z


def q_actions(L, y, eps, seed, gid0, episode, step):
    """(action[n] int32, explored[n] bool) of the Q head on outputs y[n][16]"""
    y, episode, step = _f32(y), _i32(episode), _i32(step)
    out, ex = np.zeros(y.shape[0], dtype=np.int32), np.zeros(y.shape[0], dtype=np.uint8)
    L.gtc_q_actions(y.shape[0], y.ctypes.data, y.shape[1], float(eps), int(seed), int(gid0), episode.ctypes.data, step.ctypes.data,
                    out.ctypes.data, ex.ctypes.data)
    return out, ex.astype(bool)


def actor_actions(L, y, eps, noise, seed, gid0, episode, step):
    """(action[n][A] float32, explored[n] bool) of the tanh head on outputs y[n][A]; noise None or [2][A] (mu, sigma)"""
    y, episode, step = _f32(y), _i32(episode), _i32(step)
    na = y.shape[1]
    nz = _f32(np.zeros((2, na)) if noise is None else noise)
    assert nz.shape == (2, na)
    out, ex = np.zeros((y.shape[0], na), dtype=F), np.zeros(y.shape[0], dtype=np.uint8)
    L.gtc_actor_actions(y.shape[0], y.ctypes.data, na, float(eps), int(noise is not None), nz.ctypes.data, int(seed), int(gid0),
                        episode.ctypes.data, step.ctypes.data, out.ctypes.data, ex.ctypes.data)
    return out, ex.astype(bool)


# ------------------------------------------------------------------------------------------------------------------ float64
def views(p, hidden, na):
    """[W_1, b_1, ..., W_out, b_out]: writable views into the packed parameter vector p (nn.Sequential order, input width 4)"""
    out, o, win = [], 0, IN
    for w in tuple(hidden) + (na,):
        for shape in ((w, win), (w,)):
            s = int(np.prod(shape))
            out.append(p[o:o + s].reshape(shape))
            o += s
        win = w
    return out


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1 - k * u)


# activation -> (float64 function, Lipschitz constant, the spec function's absolute error against it), as tests/wide_f64.py
ACTS = {'relu': (lambda v: np.maximum(v, 0.0), 1.0, 0.0),
        'tanh': (np.tanh, 1.0, 1e-6),
        'sigmoid': (lambda v: 1.0 / (1.0 + np.exp(-v)), 0.25, SIGMOID_ERR)}


def f64_bound(params, x, hidden, na, act):
    """y64 (the network in float64 on the same float32 inputs) and a rigorous bound on |y - y64| per output.  Per layer a k-ordered
    fmaf chain of K terms (K = 4 in layer 1: no pad; then the width below) gives e_pre = |W| e + gamma_K (|b| + |W| (|a| + e)) +
    K 2^-149 (the standard bound of a recursive sum of K products, each fmaf one rounding, plus the subnormal floor); behind every
    hidden unit the activation carries it on with its Lipschitz constant (relu, tanh: 1; sigmoid: 1/4) and adds the spec
    function's own stated error against float64 (relu: none; tanh_spec: 1e-6; sigmoid_spec: 1e-7)."""
    fn, lip, err = ACTS[act]
    v = [t.astype(np.float64) for t in views(np.array(params, dtype=F), hidden, na)]
    a, e, K = x.astype(np.float64), np.zeros(x.shape), IN
    for l, (Wl, b) in enumerate(zip(v[0::2], v[1::2])):
        pre = a @ Wl.T + b
        e = e @ np.abs(Wl).T + gamma(K) * (np.abs(b) + (np.abs(a) + e) @ np.abs(Wl).T) + K * 2.0 ** -149
        if l < len(hidden):
            a, e = fn(pre), lip * e + err
        else:
            a = pre
        K = Wl.shape[0]
    return a, e


def random_net(rs, hidden, na, scale=1.0):
    """weights and biases N(0, scale^2 / fan_in)"""
    p = np.zeros(param_count(hidden, na), dtype=F)
    fans = [f for w in (IN,) + tuple(hidden) for f in (w, w)]
    for v, fan in zip(views(p, hidden, na), fans):
        v[...] = rs.normal(0, scale / np.sqrt(fan), v.shape)
    return p


# -------------------------------------------------------------------------------------------------------------- closed loop
MODES = {'discrete': dict(continuous=0), 'continuous': dict(continuous=1), 'turn1': dict(continuous=1, turn=1, actor_out_size=1),
         'turn4': dict(continuous=1, turn=1, actor_out_size=4),
         'turn4_useturn': dict(continuous=1, turn=1, use_turn=1, actor_out_size=4)}


def make_oracle(n, **kw):
    """an f32 GoToCenter oracle (tests/test_gtc.py) that remembers its config, reset"""
    from test_gtc import GtcOracle, gtc_cfg
    cfg = gtc_cfg(**kw)
    orc = GtcOracle(cfg, n, 'f32')
    orc.cfg = cfg
    orc.reset()
    return orc


def closed_loop(L, orc, T, params, hidden, act, eps, noise=None, seed=0x5EED, gid0=0):
    """T steps of the oracle `orc` (tests/test_gtc.py GtcOracle, f32, already reset) driven by the restatement's actions on the
    oracle's own observations.  The head follows the oracle's mode.  Returns the records, time-major: obs, action, reward,
    done, result, terminal_obs (the observation the episode ended on; zeros where not done) and explored."""
    n = orc.n
    cont = bool(orc_continuous(orc))
    na = 16 if not cont else orc_adim(orc)
    turn_mode = bool(orc.cfg.turn and orc.cfg.continuous)        # rollout()'s action record: [T][N][A] in the turn mode, else [T][N]
    rec = dict(obs=np.zeros((T, n, 4), F), action=np.zeros((T, n, na) if turn_mode else (T, n), F if cont else np.int32),
               reward=np.zeros((T, n), F), done=np.zeros((T, n), np.uint8), result=np.zeros((T, n), np.uint8),
               terminal_obs=np.zeros((T, n, 4), F), explored=np.zeros((T, n), bool))
    for t in range(T):
        y = forward(L, orc.obs(), params, hidden, na, act)
        ep, st = orc.get('episode'), orc.get('step_count')
        if cont:
            a, ex = actor_actions(L, y, eps, noise, seed, gid0, ep, st)
        else:
            a, ex = q_actions(L, y, eps, seed, gid0, ep, st)
        orc.step(a, None)
        done = orc.get('done')
        rec['obs'][t], rec['reward'][t], rec['done'][t], rec['result'][t] = orc.obs(), orc.get('reward'), done, orc.get('result')
        rec['action'][t] = a if (turn_mode or not cont) else a[:, 0]
        rec['explored'][t] = ex
        d = done.astype(bool)
        term = orc.obs(terminal=True) if orc_auto_reset(orc) else orc.obs()
        rec['terminal_obs'][t][d] = term[d]
    return rec


def orc_continuous(orc):
    return orc.cfg.continuous


def orc_adim(orc):
    return int(orc.cfg.actor_out_size) if (orc.cfg.turn and orc.cfg.continuous) else 1


def orc_auto_reset(orc):
    return bool(orc.cfg.auto_reset)


# the inputs of the closed-loop tests: N not a multiple of 64, T = 120 at max_steps = 50 (every env finishes episodes and starts
# new ones), a network per mode with N(0, 9 / fan_in) weights (tests/test_gtc_actor_host.py shows that Goal, Out and Timeout all
# occur with them) and a Gaussian noise row per output
LOOP_N, LOOP_T = 1000, 120


def loop_net(mode):
    """(hidden, activation, outputs, params) of the closed-loop network of `mode`"""
    kw = MODES[mode]
    na = 16 if not kw['continuous'] else kw.get('actor_out_size', 1)
    hidden, act = {'discrete': ((64, 64), 'relu'), 'continuous': ((16, 8), 'tanh'), 'turn1': ((20,), 'sigmoid'),
                   'turn4': ((28, 16), 'relu'), 'turn4_useturn': ((16, 8), 'tanh')}[mode]
    rs = np.random.RandomState(sorted(MODES).index(mode))
    return hidden, act, na, random_net(rs, hidden, na, 3.0)


def loop_noise(na):
    return np.array([[0.05, -0.05, 0.0, 0.1][:na], [0.2, 0.3, 0.1, 0.5][:na]], dtype=F)
