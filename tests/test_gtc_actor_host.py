"""CPU checks of the GoToCenter fused actors' host side (include/s2d_gtc.h s2d_gtc_rollout_qnet / s2d_gtc_rollout_actor): the plan's
arithmetic against the C plan, the restatement of the 4-input network (tests/gtc_actor_ref.c) against numpy float64, the -0 rule
of its unpadded layer 1, GtcQNetActor / GtcDeterministicActor packing and refusals, the heads' draws, and a closed loop of the
restatement through the GoToCenter oracle."""
import ctypes as C
import re

import numpy as np
import pytest

import gtc_actor_ref as R

torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32

# quantiles at 1 - 1e-6, as tests/test_gpu_distributions.py's P_TAIL: chi-square with one degree of freedom, and the two-sided
# standard normal (scipy.stats.chi2.ppf(1 - 1e-6, 1) = 23.928; its square root 4.8916 = norm.ppf(1 - 0.5e-6))
CHI2_1DOF = 23.928
Z_TWO_SIDED = 4.8916


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp('gtc_actor_ref'))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi, gtc
    return gtc.bind(_capi.load_library())


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


# ----------------------------------------------------------------------------------------------------------------------- plan
# (hidden, outputs) -> (waves, env tiles, LDS bytes, workspace bytes), worked by hand.  Per wave W(T) = 32 T pitch + 64 (A16 + 4) +
# 256 words (no prepared-episode tile, an observation tile of 64 x 4), pitch = the widest padded layer rounded up to 64, + 4; LDS =
# 4 (B + waves W(T)) <= 163840, B = the widths and A each rounded up to 16.  Workspace = 4 (64 F + B), F = sum over the layers of
# ceil(h_l / 16) * ksteps_l with ksteps 1 for layer 1, then h_(l-1) / 4.
PLAN_TABLE = (
    # pitch 68, B = 144: W(4) = 8704 + 1280 + 256 = 10240 -> 4 (144 + 40960) = 164416, 576 bytes too much; W(2) = 4352 + 1536 = 5888
    # -> 4 (144 + 23552) = 94784.  F = 4 + 4 * 16 + 16 = 84: 4 (5376 + 144) = 22080
    (((64, 64), 16), (4, 2, 94784, 22080)),
    # pitch 68, B = 16 + 16 + 16 = 48: W(4) = 10240 -> 4 (48 + 40960) = 164032 too much; W(2): 4 (48 + 23552) = 94400.
    # F = 1 + 1 * 4 + 1 * 2 = 7: 4 (448 + 48) = 1984
    (((16, 8), 4), (4, 2, 94400, 1984)),
    # pitch 452, B = 400 + 304 + 16 = 720: W(1) = 14464 + 1280 + 256 = 16000; 4 waves 4 (720 + 64000) = 258880 too much; 2 waves
    # W(4) = 59392, W(2) = 30464 too much (4 (720 + 60928) = 246592), W(1): 4 (720 + 32000) = 130880.
    # F = 25 + 19 * 100 + 75 = 2000: 4 (128000 + 720) = 514880
    (((400, 300), 1), (2, 1, 130880, 514880)),
    # pitch 452, B = 2016: 2 waves W(1): 4 (2016 + 32000) = 136064.  F = 25 + 4 * 25 * 100 + 100 = 10125: 4 (648000 + 2016)
    (((400,) * 5, 16), (2, 1, 136064, 2600064)),
)
GRID = ([(w,) * L for w in (8, 16, 32, 64, 128, 256, 400) for L in range(1, 6)] +
        [(16, 8), (64, 64), (400, 300), (12,), (20,), (28,), (28, 16), (12, 20, 28)])


def _shape(hidden, na):
    from soccer2d_amd import _capi
    s = _capi.S2DWideNet()
    s.n_hidden = len(hidden)
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    s.n_out = na
    return s


def test_plan_equals_the_c_plan(lib):
    from soccer2d_amd.gtc_actor import LDS_BYTES, gtc_plan
    for (hidden, na), want in PLAN_TABLE:
        assert gtc_plan(hidden, na) == want, (hidden, na, gtc_plan(hidden, na))
    for hidden in GRID:
        for na in (1, 2, 3, 4, 16):
            waves, tiles, nbytes, ws = gtc_plan(hidden, na)
            assert nbytes <= LDS_BYTES and waves in (1, 2, 4) and tiles in (1, 2, 4)
            assert lib.s2d_gtc_actor_workspace_bytes(C.byref(_shape(hidden, na))) == ws, (hidden, na)
            from soccer2d_amd.gtc_actor import param_count
            assert ws >= 4 * param_count(hidden, na)
    for hidden in ((404,), (6,), (18,), (0,), (64, 7)):
        assert lib.s2d_gtc_actor_workspace_bytes(C.byref(_shape(hidden, 16))) == 0
    bad = _shape((64,), 16)
    bad.hidden[1] = 8                                                           # an entry past n_hidden
    assert lib.s2d_gtc_actor_workspace_bytes(C.byref(bad)) == 0
    bad = _shape((64,), 16)
    bad.n_hidden = 6
    assert lib.s2d_gtc_actor_workspace_bytes(C.byref(bad)) == 0
    assert lib.s2d_gtc_actor_workspace_bytes(C.byref(_shape((64,), 0))) == 0
    assert lib.s2d_gtc_actor_workspace_bytes(C.byref(_shape((64,), 65))) == 0
    assert lib.s2d_gtc_actor_workspace_bytes(None) == 0


def test_plan_takes_the_pairs_in_the_stated_order():
    """more waves before more tiles: (4, 4), (4, 2), (4, 1), (2, 4), ..."""
    from soccer2d_amd.gtc_actor import gtc_plan
    assert gtc_plan((8,), 1)[:2] == (4, 2)            # even the smallest shape: 4 x W(4) = 4 x 10240 words is the whole LDS
    assert gtc_plan((256, 256), 16)[:2] == (4, 1)      # 4 (528 + 4 x 9856) = 159808; (4, 2) would need 292928


def test_new_symbols_are_bound_and_exported(lib):
    from soccer2d_amd import gtc
    names = {p[0]: p for p in gtc.GTC_PROTOTYPES}
    for name, nargs in (('s2d_gtc_actor_workspace_bytes', 1), ('s2d_gtc_rollout_qnet', 6), ('s2d_gtc_rollout_actor', 6),
                        ('s2d_gtc_debug_forward', 7), ('s2d_gtc_kernel_name', 1)):
        assert name in names and len(names[name][2]) == nargs
        assert getattr(lib, name) is not None


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('hidden', [(8,), (12,), (28, 16), (16, 8), (64, 64), (400, 300), (8, 400, 12, 300, 16)],
                         ids=lambda h: '-'.join(map(str, h)))
def test_restatement_against_float64(ref, hidden):
    """every output of gtc_actor_ref lies within the rigorous running bound (gtc_actor_ref.f64_bound) of the float64 network, for
    the three activations; the bound is what the number formats and the activations' stated errors give, nothing is fitted"""
    rs = np.random.RandomState(sum(hidden))
    for act, na in (('relu', 16), ('tanh', 4), ('sigmoid', 3)):
        p = R.random_net(rs, hidden, na)
        x = rs.uniform(-1, 1, (64, 4)).astype(F)
        y = R.forward(ref, x, p, hidden, na, act)
        y64, e = R.f64_bound(p, x, hidden, na, act)
        assert (np.abs(y - y64) <= e).all(), (act, float((np.abs(y - y64) / e).max()))
        assert len(np.unique(y)) > 32


def minus_zero_case(hidden=(8,), na=2):
    """(params, x): layer 1 with -0 biases and -0 weights on positive inputs -- every product is -0, so every accumulator stays
    -0 through the four terms; tanh_spec(-0) = -0; the output layer has -0 biases and weights +1 on unit 0, +0 elsewhere:
    fmaf(+w, -0, -0) = -0.  A padded layer 1 (two more fmaf(+0, +0, acc)) would give +0 instead."""
    p = np.zeros(R.param_count(hidden, na), dtype=F)
    v = R.views(p, hidden, na)
    for t in v[:2 * len(hidden)]:
        t[...] = -0.0
    v[-2][...] = 0.0
    v[-2][:, 0] = 1.0
    v[-1][...] = -0.0
    x = np.array([[0.5, 1.0, 0.25, 2.0]], dtype=F)
    return p, x


def test_minus_zero_stays_minus_zero(ref):
    p, x = minus_zero_case()
    y = R.forward(ref, x, p, (8,), 2, 'tanh')
    assert np.array_equal(bits(y), bits(np.array([[-0.0, -0.0]], dtype=F)))
    # the same parameters through relu: -0 -> +0 behind layer 1, and the output is fmaf(1, +0, -0) = +0
    assert np.array_equal(bits(R.forward(ref, x, p, (8,), 2, 'relu')), bits(np.zeros((1, 2), dtype=F)))


def test_special_values_of_the_restatement(ref):
    hidden, na = (8,), 1
    p = np.zeros(R.param_count(hidden, na), dtype=F)
    v = R.views(p, hidden, na)
    v[0][0, :] = [1e-20, 0, 0, 0]                 # a subnormal survives: 1e-20 * 1e-20 = 1e-40
    v[2][0, 0] = 1.0
    y = R.forward(ref, np.array([[1e-20, 0, 0, 0]], dtype=F), p, hidden, na, 'relu')
    assert y[0, 0] == F(1e-20) * F(1e-20) and 0 < y[0, 0] < 2.0 ** -126
    y = R.forward(ref, np.array([[np.inf, 0, 0, 0]], dtype=F), p, hidden, na, 'tanh')      # inf * 0 in the chain -> NaN
    assert np.isnan(y[0, 0])
    assert R.forward(ref, np.array([[np.nan, 0, 0, 0]], dtype=F), p, hidden, na, 'relu')[0, 0] == 0.0   # relu(NaN) = +0


# -------------------------------------------------------------------------------------------------------------------- classes
_ACT = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}


def _seq(hidden, na, act=nn.ReLU, tanh_head=False, n_in=4, flatten=False):
    layers, win = ([nn.Flatten()] if flatten else []), n_in
    for w in hidden:
        layers += [nn.Linear(win, w), act()]
        win = w
    layers.append(nn.Linear(win, na))
    if tanh_head:
        layers.append(nn.Tanh())
    return nn.Sequential(*layers)


def test_from_module_round_trip():
    from soccer2d_amd.gtc_actor import GtcDeterministicActor, GtcQNetActor, gtc_plan, param_count
    torch.manual_seed(0)
    cases = ((GtcQNetActor, (64, 64), 'relu', 16, False),                    # SB3's DQN default
             (GtcDeterministicActor, (16, 8), 'relu', 4, True),              # the script's pi: [16, 8], turn mode
             (GtcDeterministicActor, (400, 300), 'sigmoid', 1, True),
             (GtcQNetActor, (32, 400, 8, 128, 64), 'tanh', 16, False))
    for cls, hidden, act, na, head in cases:
        net = _seq(hidden, na, _ACT[act], tanh_head=head, flatten=not head)
        a = cls.from_module(net, device='cpu')
        want, win = [], 4
        for w in hidden + (na,):
            want += [(w, win), (w,)]
            win = w
        assert a.shapes() == tuple(want) and a.in_dim == 4
        assert a.hidden == hidden and a.activation == act
        flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
        assert a.params.shape == (param_count(hidden, na),) == flat.shape and torch.equal(a.params, flat)
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.5)
        assert torch.equal(a.params, flat)
        a.sync()
        assert torch.equal(a.params, torch.cat([p.detach().reshape(-1) for p in net.parameters()]))
        s = a.c_struct()
        assert s.n_hidden == len(hidden) and list(s.hidden) == list(hidden) + [0] * (5 - len(hidden))
        assert s.n_out == na and s.activation == ('relu', 'tanh', 'sigmoid').index(act) and s.noise_kind == 0
        assert s.workspace_bytes == gtc_plan(hidden, na)[3] == a.workspace.numel() * 4 and a.plan == gtc_plan(hidden, na)
        a.epsilon = 0.25
        assert a.epsilon == 0.25 and float(a.epsilon_tensor) == 0.25
        # load_from on a second module of the same shape
        other = _seq(hidden, na, _ACT[act], tanh_head=head)
        a.load_from(other)
        assert torch.equal(a.params, torch.cat([p.detach().reshape(-1) for p in other.parameters()]))
    d = GtcDeterministicActor.from_module(_seq((16, 8), 4, tanh_head=True), device='cpu', noise_sigma=0.2, noise_mean=0.1)
    assert d.noise_kind == 1 and d.c_struct().noise_kind == 1
    assert d.noise_sigma.tolist() == pytest.approx([0.2] * 4) and d.noise_mean.tolist() == pytest.approx([0.1] * 4)


def test_refusals():
    from soccer2d_amd.gtc_actor import GtcDeterministicActor, GtcQNetActor
    mixed = nn.Sequential(nn.Linear(4, 32), nn.ReLU(), nn.Linear(32, 32), nn.Sigmoid(), nn.Linear(32, 16))
    cases = ((_seq((64, 64), 16, n_in=10), 'in_features = 4'),
             (mixed, 'one activation'),
             (_seq((32, 32), 16, nn.GELU), 'ReLU, Tanh or Sigmoid'),
             (_seq((404,), 16), 'multiple of 4'),
             (_seq((6,), 16), 'multiple of 4'),
             (_seq((64, 18), 16), 'multiple of 4'),
             (_seq((), 16), 'hidden layers'),
             (_seq((32,) * 6, 16), 'hidden layers'),
             (_seq((64, 64), 8), '16 outputs'))
    for net, word in cases:
        with pytest.raises(ValueError, match=re.escape(word)):
            GtcQNetActor.from_module(net, device='cpu')
    with pytest.raises(ValueError, match=re.escape('in_features = 4')):
        GtcDeterministicActor.from_module(_seq((16, 8), 1, tanh_head=True, n_in=10), device='cpu')
    with pytest.raises(ValueError, match='Tanh'):
        GtcDeterministicActor.from_module(_seq((16, 8), 1), device='cpu')             # no tanh head
    with pytest.raises(ValueError, match='n_out'):
        GtcDeterministicActor.from_module(_seq((16, 8), 5, tanh_head=True), device='cpu')
    with pytest.raises(ValueError, match='activation'):
        GtcQNetActor((64, 64), activation='gelu', device='cpu')
    with pytest.raises(ValueError, match='activation'):
        GtcQNetActor((64, 64), activation='sigmoid', device='cpu').load_from(_seq((64, 64), 16, nn.Tanh))
    with pytest.raises(ValueError, match='shapes'):
        GtcQNetActor((64, 64), device='cpu').load_from(_seq((64, 64), 16, n_in=10))
    for hidden in ((404,), (6,), (18,), (32,) * 6):
        with pytest.raises(ValueError):
            GtcQNetActor(hidden, device='cpu')


# ---------------------------------------------------------------------------------------------------------------------- heads
N_DRAWS = 65536


def test_threshold_and_explore_rate(ref):
    assert ref.gtc_threshold(0.0) == 0 and ref.gtc_threshold(-1.0) == 0 and ref.gtc_threshold(float('nan')) == 0
    assert ref.gtc_threshold(1.0) == 1 << 32 and ref.gtc_threshold(2.0) == 1 << 32
    assert ref.gtc_threshold(0.5) == 1 << 31
    rs = np.random.RandomState(0)
    y = rs.normal(size=(N_DRAWS, 16)).astype(F)
    ep, st = rs.randint(0, 50, N_DRAWS), rs.randint(0, 200, N_DRAWS)
    greedy = R.argmax(ref, y)
    a0, ex0 = R.q_actions(ref, y, 0.0, 0x5EED, 0, ep, st)
    assert not ex0.any() and np.array_equal(a0, greedy)                        # epsilon = 0 never explores
    a1, ex1 = R.q_actions(ref, y, 1.0, 0x5EED, 0, ep, st)
    assert ex1.all() and np.bincount(a1, minlength=16).min() > 0               # epsilon = 1 always does
    _, ex = R.q_actions(ref, y, 0.3, 0x5EED, 0, ep, st)
    p = float(F(0.3))
    stat = (ex.sum() - N_DRAWS * p) ** 2 / (N_DRAWS * p * (1 - p))
    assert stat < CHI2_1DOF, (ex.mean(), stat)
    # the words are those of stream 9, and differ from key to key
    w = R.explore_words(ref, 0x5EED, 0, ep, st)
    assert np.array_equal(ex, w.astype(np.uint64) < np.uint64(ref.gtc_threshold(0.3))) and len(np.unique(w)) > N_DRAWS - 8
    # the tanh head: the same decisions, the random policy's action when exploring, tanh_spec(y) else
    ya = rs.normal(size=(N_DRAWS, 4)).astype(F)
    act, exa = R.actor_actions(ref, ya, 0.3, None, 0x5EED, 0, ep, st)
    assert np.array_equal(exa, ex)
    assert np.abs(act[~exa] - np.tanh(ya[~exa].astype(np.float64))).max() <= 1e-6 and (np.abs(act) <= 1).all()


def test_argmax_ties_and_nan(ref):
    y = np.zeros((4, 16), dtype=F)
    y[1, [3, 7]] = 1.0                         # a tie: the lowest index
    y[2, 0], y[2, 5] = np.nan, 1.0             # q[0] = NaN is never beaten (v > NaN is false): index 0 stays
    y[3, 5], y[3, 9] = np.nan, 2.0             # a NaN never wins
    assert R.argmax(ref, y).tolist() == [0, 3, 0, 9]


def test_gaussian_noise_moments(ref):
    rs = np.random.RandomState(1)
    ep, st = rs.randint(0, 50, N_DRAWS), rs.randint(0, 200, N_DRAWS)
    z = R.gauss(ref, 0x5EED, 0, ep, st).astype(np.float64)
    n = z.size
    assert abs(z.mean()) * np.sqrt(n) < Z_TWO_SIDED                                    # mean 0: variance 1 / n
    assert abs((z ** 2).mean() - 1.0) * np.sqrt(n / 2.0) < Z_TWO_SIDED                 # E z^2 = 1: var z^2 = 2
    for j in range(4):                                                                 # each of z0 .. z3 on its own
        assert abs(z[:, j].mean()) * np.sqrt(N_DRAWS) < Z_TWO_SIDED
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) * np.sqrt(N_DRAWS) < Z_TWO_SIDED
    # the head adds mu + sigma z and clips
    y = rs.normal(size=(N_DRAWS, 4)).astype(F)
    noise = np.array([[0.1, -0.1, 0.0, 0.2], [0.2, 0.3, 0.0, 1.5]], dtype=F)
    act, ex = R.actor_actions(ref, y, 0.0, noise, 0x5EED, 0, ep, st)
    plain, _ = R.actor_actions(ref, y, 0.0, None, 0x5EED, 0, ep, st)
    assert not ex.any() and (np.abs(act) <= 1).all() and (np.abs(act[:, 3]) == 1).any()
    assert np.array_equal(bits(act[:, 2]), bits(plain[:, 2] + F(0.0)))                 # sigma = mu = 0: a + 0
    inside = np.abs(act[:, 0]) < 1
    want = plain[:, 0].astype(np.float64) + 0.1 + 0.2 * z[:, 0]
    assert np.abs(act[inside, 0] - want[inside]).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------- closed loop
@pytest.mark.parametrize('mode', list(R.MODES))
def test_closed_loop_reaches_every_result(ref, mode):
    """the inputs of the GPU closed-loop test (tests/test_gpu_gtc_actor.py) exercise Goal, Out and Timeout in every mode"""
    kw = R.MODES[mode]
    hidden, act, na, p = R.loop_net(mode)
    for eps, noise in ((0.0, None), (0.3, R.loop_noise(na) if kw['continuous'] else None)):
        orc = R.make_oracle(R.LOOP_N, max_steps=50, **kw)
        rec = R.closed_loop(ref, orc, R.LOOP_T, p, hidden, act, eps, noise)
        counts = np.bincount(rec['result'].ravel(), minlength=4)
        assert (counts[1:] > 0).all(), (mode, eps, counts)
        assert list(orc.stats()[:4]) == [R.LOOP_N * R.LOOP_T] + list(counts[1:])
        assert (rec['explored'].any() if eps else not rec['explored'].any())
        d = rec['done'].astype(bool)
        assert (rec['terminal_obs'][d] != 0).any(axis=-1).all() and not rec['terminal_obs'][~d].any()
