"""The device replay buffer on the GPU (s2d_replay_push / s2d_replay_sample through soccer2d_amd.replay.DeviceReplay): every ring
word and the cursor against the host restatement (tests/replay_ref.c) over the wave edges, both copy widths and the ring's wrap;
sampled batches and their uniformity; closed loops with the reach-ball and GoToCenter fused actors, where a 1-step push also
equals the examples' torch formulation; push + sample in one captured graph; rejections.  Every comparison is bitwise."""
import ctypes as C
import itertools

import numpy as np
import pytest

import replay as RR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
SENTINEL = 0xA5A5A5A5
GAMMA = 0.97


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return RR.build(tmp_path_factory.mktemp('replay_ref'))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def words_of(t):
    """a 4-byte device tensor as int32 words"""
    return t.view(torch.int32)


def dev_rec(rec):
    return {k: torch.from_numpy(v).to(DEV) for k, v in rec.items()}


def host_rec(rec):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in rec.items() if torch.is_tensor(v)}


def twin(capacity, D, AW, float_action, n_step=1, gamma=GAMMA, seed=0, fill=SENTINEL, cursor=(0, 0, 0, 0)):
    """a DeviceReplay and a host ring in the same state: every word the sentinel, the same cursor"""
    from soccer2d_amd.replay import DeviceReplay
    rb = DeviceReplay(capacity, D, action_words=AW, action_dtype=torch.float32 if float_action else torch.int32, device=DEV,
                      n_step=n_step, gamma=gamma, seed=seed)
    ring = RR.Ring(capacity, D, AW, fill=fill)
    for k in RR.RING_FIELDS:
        words_of(getattr(rb, k)).fill_(int(np.uint32(fill).view(np.int32)))
    ring.cursor[:] = cursor
    rb.cursor.copy_(torch.tensor(cursor, dtype=torch.int64))
    return rb, ring


def load_ring(rb, ring):
    """the host ring's contents and cursor into the device buffer"""
    for k in RR.RING_FIELDS:
        words_of(getattr(rb, k)).copy_(torch.from_numpy(bits(getattr(ring, k)).view(np.int32)))
    rb.cursor.copy_(torch.from_numpy(ring.cursor.astype(np.int64)))


def same_ring(rb, ring, what):
    torch.cuda.synchronize()
    for k in RR.RING_FIELDS:
        got, want = bits(getattr(rb, k).cpu().numpy()).reshape(ring.capacity, -1), bits(getattr(ring, k)).reshape(ring.capacity, -1)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f'{what}: {k} differs in {bad.size} slots, first {bad[:5]}'
    assert rb.cursor.cpu().tolist() == ring.cursor.tolist(), what


def same_batch(got, want, what):
    torch.cuda.synchronize()
    for k in RR.BATCH_FIELDS:
        g, w = bits(got[k].cpu().numpy()).reshape(len(want['index']), -1), bits(want[k]).reshape(len(want['index']), -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, f'{what}: {k} differs in {bad.size} elements, first {bad[:5]}'


# ------------------------------------------------------------------------------------------ push against the restatement
def _grid():
    """a pruned product: every (N, T) pair twice, the other axes cycled so that every D and every n_step meets every N and every T"""
    Ns, Ts, Ds, AWs, cases = (1, 63, 64, 65, 257), (1, 2, 5, 9), (1, 4, 10, 17, 224), (1, 4), []
    for (a, N), (b, T) in itertools.product(enumerate(Ns), enumerate(Ts)):
        steps = (1, 2, 3, T + 2)
        for rep in range(2):
            cases.append((N, T, steps[(3 * a + b + rep) % 4], Ds[(a + b + 2 * rep) % 5], AWs[(a + b // 2 + rep) % 2]))
    return cases


GRID = _grid()


def test_grid_covers_every_value():
    for axis, values in ((0, {1, 63, 64, 65, 257}), (1, {1, 2, 5, 9}), (3, {1, 4, 10, 17, 224}), (4, {1, 4})):
        assert {c[axis] for c in GRID} == values
    assert {c[2] for c in GRID} >= {1, 2, 3} and any(c[2] == c[1] + 2 for c in GRID) and 30 <= len(GRID) <= 60
    assert any(c[0] == 257 and c[3] == 224 for c in GRID) and any(c[0] == 65 and c[3] % 4 == 0 for c in GRID)


@pytest.mark.parametrize('N,T,n_step,D,AW', GRID)
def test_push_equals_restatement_every_ring_word_and_the_cursor(L, N, T, n_step, D, AW):
    rng = np.random.default_rng(1000 * N + 10 * T + D)
    cap = T * N + 37
    pos = int(rng.integers(0, cap))
    rec, first = RR.synthetic_record(rng, T, N, D, AW, float_action=AW == 4)
    rb, ring = twin(cap, D, AW, AW == 4, n_step=n_step, cursor=(pos, 5, 2, 1))
    rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
    RR.push(L, ring, rec, first, n_step, GAMMA)
    assert (ring.obs[(pos + T * N) % cap] == SENTINEL).all()            # untouched slots exist and stay the sentinel
    same_ring(rb, ring, f'N={N} T={T} n={n_step} D={D} AW={AW} pos={pos}')


def test_push_without_result_terminates_every_done(L):
    rng = np.random.default_rng(3)
    rec, first = RR.synthetic_record(rng, 5, 70, 10, 1, with_result=False)
    rb, ring = twin(400, 10, 1, False, n_step=3)
    rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
    RR.push(L, ring, rec, first, 3, GAMMA)
    same_ring(rb, ring, 'no result')
    assert rec['done'].any() and not ring.discount[:350][rec['done'].reshape(-1) != 0].any()


# ------------------------------------------------------------------------------------------ wrap
@pytest.mark.parametrize('D', [4, 10])
def test_push_straddles_the_rings_end_inside_a_wave(L, D):
    rng = np.random.default_rng(4)
    T, N, cap = 2, 100, 300
    rec, first = RR.synthetic_record(rng, T, N, D, 1)
    rb, ring = twin(cap, D, 1, False, n_step=2, cursor=(cap - 70, 300, 9, 0))     # transition 70 (wave 1, lane 6) lands in slot 0
    rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
    RR.push(L, ring, rec, first, 2, GAMMA)
    assert ring.cursor.tolist() == [130, 300, 10, 0] and (ring.obs[130:cap - 70] == SENTINEL).all()
    same_ring(rb, ring, f'wrap D={D}')


@pytest.mark.parametrize('cap', [200, 250])
def test_two_pushes_overwrite_the_oldest_slots(L, cap):
    """capacity == T * N exactly (every push rewrites the whole ring from pos 0) and a capacity the second push wraps in"""
    rng = np.random.default_rng(cap)
    T, N, D = 2, 100, 10
    rb, ring = twin(cap, D, 1, False)
    for n in range(2):
        rec, first = RR.synthetic_record(rng, T, N, D, 1)
        rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
        RR.push(L, ring, rec, first, 1, GAMMA)
        same_ring(rb, ring, f'cap={cap} push {n}')
    assert ring.cursor.tolist() == [400 % cap, cap, 2, 0] and (rb.pos, rb.size) == (400 % cap, cap)
    assert not (ring.obs == SENTINEL).any()


def raw_push(lib, rb, rec, first, result=True):
    T, N = rec['reward'].shape
    p = [C.c_void_p(t.data_ptr()) for t in (first, rec['obs'], rec['terminal_obs'], rec['action'], rec['reward'], rec['done'])]
    return lib.s2d_replay_push(T, N, rb.obs_dim, rb.action_words, rb.n_step, rb.gamma, *p,
                               C.c_void_p(rec['result'].data_ptr()) if result else None, C.byref(rb._ring),
                               C.c_void_p(rb.cursor.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_one_transition_too_many_is_einval_and_touches_nothing(L):
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    rng = np.random.default_rng(5)
    T, N, D = 3, 67, 4
    rec, first = RR.synthetic_record(rng, T, N, D, 1)
    rb, ring = twin(T * N - 1, D, 1, False, cursor=(7, 3, 1, 0))
    d, f = dev_rec(rec), torch.from_numpy(first).to(DEV)
    assert raw_push(lib, rb, d, f) == _capi.S2D_EINVAL and b'capacity' in lib.s2d_last_error()
    with pytest.raises(ValueError, match='capacity'):
        rb.push(d, f)
    same_ring(rb, ring, 'T * N = C + 1')
    rb2, ring2 = twin(T * N, D, 1, False, cursor=(7, 3, 1, 0))                       # one slot more: accepted
    assert raw_push(lib, rb2, d, f) == 0
    RR.push(L, ring2, rec, first, 1, GAMMA)
    same_ring(rb2, ring2, 'T * N = C')


# ------------------------------------------------------------------------------------------ sample
def random_ring(rng, cap, D, AW, cursor):
    ring = RR.Ring(cap, D, AW)
    for k in RR.RING_FIELDS:
        a = bits(getattr(ring, k))
        a[...] = rng.integers(0, 2 ** 32, a.shape, dtype=np.uint64).astype(np.uint32)
    ring.cursor[:] = cursor
    return ring


@pytest.mark.parametrize('D,AW', [(10, 1), (4, 4), (224, 1)])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 1000])
def test_sample_equals_restatement(L, B, D, AW):
    rng = np.random.default_rng(B + D)
    cap, seed = 311, 0xFEDCBA9876543210
    for size in (1, 7, cap):
        ring = random_ring(rng, cap, D, AW, (11, size, 3, 5))
        rb, _ = twin(cap, D, AW, AW == 4, seed=seed)
        load_ring(rb, ring)
        first, second = rb.sample(B), rb.sample(B)
        w1, w2 = RR.sample(L, ring, B, seed), RR.sample(L, ring, B, seed)
        same_batch(first, w1, f'B={B} size={size} call 0')
        same_batch(second, w2, f'B={B} size={size} call 1')
        same_ring(rb, ring, f'B={B} size={size}: sampling changes only the sample counter')
        assert ring.cursor[3] == 7 and 0 <= w1['index'].min() and w1['index'].max() < size
        if size > 1 and B > 1:
            assert not np.array_equal(w1['index'], w2['index'])


def test_sample_of_an_empty_buffer_is_the_zero_batch(L):
    rng = np.random.default_rng(6)
    ring = random_ring(rng, 100, 10, 2, (0, 0, 0, 0))
    rb, _ = twin(100, 10, 2, False)
    load_ring(rb, ring)
    out = rb.alloc_batch(130)
    for k in RR.BATCH_FIELDS:
        words_of(out[k]).fill_(0x1234567)
    got = rb.sample(130, out=out)
    assert got is out
    same_batch(got, RR.sample(L, ring, 130, 0), 'empty')
    assert (out['index'] == -1).all() and not any(words_of(out[k]).any() for k in RR.RING_FIELDS)
    assert rb.cursor.cpu().tolist() == [0, 0, 0, 1]


def test_sample_is_uniform(L):
    """B = 65 536 draws over 64 slots: chi-square below its 1 - 1e-6 quantile (the convention of test_gpu_distributions.py)"""
    chi2 = pytest.importorskip('scipy.stats').chi2
    rb, _ = twin(64, 1, 1, False, seed=12345, cursor=(0, 64, 1, 0))
    idx = rb.sample(65536)['index'].cpu().numpy()
    assert idx[::257].tolist() == [L.replay_index(12345, 0, b, 64) for b in range(0, 65536, 257)]
    counts = np.bincount(idx, minlength=64).astype(np.float64)
    stat = float(((counts - 1024.0) ** 2 / 1024.0).sum())
    limit = float(chi2.ppf(1.0 - 1e-6, 63))
    assert idx.min() == 0 and idx.max() == 63
    assert stat < limit, f'chi2 = {stat:.1f} with 63 degrees of freedom exceeds the 1 - 1e-6 quantile {limit:.1f}'


# ------------------------------------------------------------------------------------------ closed loops with real engines
def _check_record(L, rec, first, D, AW, float_action, what):
    """push the device record with n_step 1 and 3 against the restatement on the copied-back record; the 1-step ring also equals
    the examples' torch formulation on the device"""
    T, N = rec['reward'].shape
    h_rec, h_first = host_rec(rec), first.cpu().numpy()
    for n_step in (1, 3):
        rb, ring = twin(T * N + 50, D, AW, float_action, n_step=n_step, gamma=0.99)
        rb.push(rec, first)
        RR.push(L, ring, h_rec, h_first, n_step, 0.99)
        same_ring(rb, ring, f'{what} n_step={n_step}')
        if n_step == 1:
            obs_t, act, rew, nxt, disc = RR.torch_formulation(rec, first, 0.99)
            for k, want in (('obs', obs_t), ('next_obs', nxt), ('action', act), ('reward', rew), ('discount', disc)):
                got = getattr(rb, k)[:T * N]
                assert torch.equal(words_of(got).reshape(T * N, -1), words_of(want.contiguous()).reshape(T * N, -1)), (what, k)
    return h_rec


def test_closed_loop_reach_ball_qnet_record(L):
    import oracle as O
    from soccer2d_amd.actor import QNetActor
    from soccer2d_amd.engine import Engine, make_config
    N, T = 300, 40
    eng = Engine(N, DEV, cfg=make_config(**dict(O.DQN_KWARGS, max_steps=12)))
    eng.reset()
    g = torch.Generator().manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 16))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.rand(p.shape, generator=g) * 2 - 1)
    actor = QNetActor.from_module(net.to(DEV), device=DEV, epsilon=0.3)
    first = eng.obs.clone()
    rec = eng.rollout_qnet(T, actor, terminal_obs=True)
    h = _check_record(L, rec, first, 10, 1, False, 'reach-ball qnet')
    counts = np.bincount(h['result'].ravel(), minlength=4)
    print('reach-ball results none/goal/out/timeout:', counts.tolist())
    assert (counts[1:] > 0).all(), counts
    assert ((h['result'] != 0) == (h['done'] != 0)).all()


def test_closed_loop_go_to_center_actor_record(L):
    from soccer2d_amd.gtc import GoToCenterVecEnv
    from soccer2d_amd.gtc_actor import GtcDeterministicActor
    N, T = 300, 40
    env = GoToCenterVecEnv(N, DEV, max_steps=12, continuous=1, turn=1, actor_out_size=4)
    env.reset()
    actor = GtcDeterministicActor((16, 8), 4, epsilon=0.5, noise_sigma=0.1)
    actor.params.copy_(torch.rand(actor.params.shape, generator=torch.Generator().manual_seed(2)) - 0.5)
    first = env.obs.clone()
    rec = env.rollout_actor(T, actor, terminal_obs=True)
    assert rec['action'].dtype == torch.float32 and tuple(rec['action'].shape) == (T, N, 4) and tuple(rec['obs'].shape) == (T, N, 4)
    h = _check_record(L, rec, first, 4, 4, True, 'GoToCenter actor')
    print('GoToCenter results none/goal/out/timeout:', np.bincount(h['result'].ravel(), minlength=4).tolist())
    assert h['done'].any()


# ------------------------------------------------------------------------------------------ graph
def test_push_then_sample_in_one_captured_graph(L):
    from soccer2d_amd import _capi
    _capi.load_library()
    rng = np.random.default_rng(9)
    T, N, D, AW, B, cap = 5, 130, 10, 1, 200, 1500                      # the third push wraps (3 * 650 > 1500)
    recs = [RR.synthetic_record(rng, T, N, D, AW) for _ in range(4)]
    rb, _ = twin(cap, D, AW, False, n_step=3, seed=77)
    eager, _ = twin(cap, D, AW, False, n_step=3, seed=77)
    rec, first = dev_rec(recs[3][0]), torch.from_numpy(recs[3][1]).to(DEV)
    batch = rb.alloc_batch(B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # a warm-up outside the capture, on a buffer of its own
        warm, _ = twin(cap, D, AW, False, n_step=3, seed=77)
        warm.push(rec, first)
        warm.sample(B)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rb.push(rec, first)
        rb.sample(B, out=batch)
    torch.cuda.synchronize()
    assert rb.cursor.cpu().tolist() == [0, 0, 0, 0]                     # capturing ran nothing
    for n in range(3):
        h_rec, h_first = recs[n]
        for k, v in h_rec.items():
            rec[k].copy_(torch.from_numpy(v))
        first.copy_(torch.from_numpy(h_first))
        graph.replay()
        torch.cuda.synchronize()
        eager.push(dev_rec(h_rec), torch.from_numpy(h_first).to(DEV))
        want = eager.sample(B)
        torch.cuda.synchronize()
        assert rb.cursor.cpu().tolist() == eager.cursor.cpu().tolist() == [(n + 1) * T * N % cap, min((n + 1) * T * N, cap), n + 1, n + 1]
        for k in RR.RING_FIELDS:
            assert torch.equal(words_of(getattr(rb, k)), words_of(getattr(eager, k))), (n, k)
        for k in RR.BATCH_FIELDS:
            assert torch.equal(words_of(batch[k]), words_of(want[k])), (n, k)
    # and the eager twin is the restatement's
    ring = RR.Ring(cap, D, AW, fill=SENTINEL)
    for n in range(3):
        RR.push(L, ring, recs[n][0], recs[n][1], 3, GAMMA)
        w = RR.sample(L, ring, B, 77)
    same_ring(eager, ring, 'three eager pushes')
    same_batch(want, w, 'third batch')


# ------------------------------------------------------------------------------------------ rejections
def test_rejections_return_einval_with_text_and_launch_nothing(L):
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    rng = np.random.default_rng(10)
    T, N, D = 3, 40, 4
    rec, first = RR.synthetic_record(rng, T, N, D, 1)
    rb, ring = twin(500, D, 1, False, cursor=(3, 2, 1, 0))
    d, f = dev_rec(rec), torch.from_numpy(first).to(DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cur = rb.cursor.data_ptr()

    def push(first=f.data_ptr(), obs=d['obs'].data_ptr(), term=d['terminal_obs'].data_ptr(), act=d['action'].data_ptr(),
             rew=d['reward'].data_ptr(), done=d['done'].data_ptr(), res=d['result'].data_ptr(), ring=rb._ring, cur=cur):
        return lib.s2d_replay_push(T, N, D, 1, 1, 0.99, first, obs, term, act, rew, done, res, C.byref(ring), cur, st)

    def ring_with(**kw):
        r = _capi.S2DReplayRing.from_buffer_copy(rb._ring)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    cases = [(dict(obs=None), b'non-NULL'), (dict(done=None), b'non-NULL'), (dict(cur=None), b'non-NULL'),
             (dict(ring=ring_with(discount=None)), b'non-NULL'),
             (dict(obs=d['obs'].data_ptr() + 4), b'16-byte'), (dict(rew=d['reward'].data_ptr() + 2), b'4-byte'),
             (dict(cur=cur + 4), b'8-byte'), (dict(ring=ring_with(next_obs=rb.next_obs.data_ptr() + 8)), b'16-byte'),
             (dict(ring=ring_with(obs=d['obs'].data_ptr())), b'overlap'),                    # the ring's obs IS the record's obs
             (dict(ring=ring_with(reward=d['reward'].data_ptr() + 8)), b'overlap'),
             (dict(term=rb.next_obs.data_ptr() + 160), b'overlap'), (dict(res=cur + 8), b'overlap'),
             (dict(ring=ring_with(next_obs=rb.obs.data_ptr())), b'overlap')]
    for kw, text in cases:
        assert push(**kw) == _capi.S2D_EINVAL, kw
        assert text in lib.s2d_last_error() and b's2d_replay_push' in lib.s2d_last_error(), (kw, lib.s2d_last_error())
    same_ring(rb, ring, 'after the refused pushes')

    B = 50
    out = rb.alloc_batch(B)
    for k in RR.BATCH_FIELDS:
        words_of(out[k]).fill_(0x7654321)

    def sample(obs=out['obs'].data_ptr(), nxt=out['next_obs'].data_ptr(), act=out['action'].data_ptr(), rew=out['reward'].data_ptr(),
               disc=out['discount'].data_ptr(), idx=out['index'].data_ptr(), cur=cur):
        return lib.s2d_replay_sample(B, D, 1, C.byref(rb._ring), cur, 1, obs, nxt, act, rew, disc, idx, st)

    for kw, text in [(dict(idx=None), b'non-NULL'), (dict(obs=out['obs'].data_ptr() + 8), b'16-byte'),
                     (dict(disc=out['discount'].data_ptr() + 1), b'4-byte'), (dict(cur=cur + 4), b'8-byte'),
                     (dict(nxt=rb.next_obs.data_ptr()), b'overlap'), (dict(idx=cur), b'overlap'),
                     (dict(rew=out['discount'].data_ptr() + 16), b'overlap')]:
        assert sample(**kw) == _capi.S2D_EINVAL, kw
        assert text in lib.s2d_last_error() and b's2d_replay_sample' in lib.s2d_last_error(), (kw, lib.s2d_last_error())
    same_ring(rb, ring, 'after the refused samples')
    assert all((words_of(out[k]) == 0x7654321).all() for k in RR.BATCH_FIELDS)
