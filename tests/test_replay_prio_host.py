"""Prioritized replay without a GPU: the host restatement (tests/replay_prio_ref.c) against a level-by-level NumPy rebuild of
the tree, hand-computed answers, the clamp, duplicates and invalid indices, the sampling rule's invariants and its
proportionality; PrioritizedReplay's argument checks on the CPU; the header, the ctypes mirror and the built library agree on the
four entry points, which reject made-up pointers before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay as RR
import replay_prio as RP
from test_capi_exports import HDR, declared_functions

NEW = ('s2d_replay_tree_words', 's2d_replay_prio_push', 's2d_replay_prio_update', 's2d_replay_sample_prio')
MIN, MAX = RP.PRIO_MIN, RP.PRIO_MAX
CHI2_63 = 131.3697020515818          # scipy.stats.chi2.ppf(1 - 1e-6, 63), the convention of test_gpu_distributions.py


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return RP.build(tmp_path_factory.mktemp('replay_prio_ref'))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cur(pos=0, size=0, pushes=0, samples=0):
    return np.array([pos, size, pushes, samples], np.uint64)


# ------------------------------------------------------------------------------------------ the tree
@pytest.mark.parametrize('cap', [1, 2, 5, 64, 100, 311])
def test_random_pushes_and_updates_keep_every_node_the_sum_of_its_children(L, cap):
    rng = np.random.default_rng(cap)
    P = RP.leaves(cap)
    tree, c = np.zeros(2 * P, np.float32), cur()
    for step in range(12):
        if step % 2 == 0:
            n = int(rng.integers(1, cap + 1))
            RP.push(L, tree, c, n, cap)
            c[0], c[1] = (c[0] + n) % cap, min(int(c[1]) + n, cap)       # what s2d_replay_push does behind it
        else:
            B = int(rng.integers(1, 40))
            idx = rng.integers(-1, cap + 1, B).astype(np.int32)
            pri = np.exp2(rng.uniform(-45, 45, B)).astype(np.float32)
            RP.update(L, tree, c, idx, pri, cap)
        assert np.array_equal(bits(tree), bits(RP.rebuilt(tree))), (cap, step)
        size = int(c[1])
        assert (tree[P:P + size] >= MIN).all() and (tree[P:P + size] <= MAX).all() and not bits(tree[P + size:]).any()
        assert tree[0] == 0 or tree[0] >= 1


def test_tree_words_and_leaves(L):
    for cap, P in ((1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (64, 64), (65, 128), (4097, 8192), (2 ** 30, 2 ** 30)):
        assert L.prio_leaves(cap) == P == RP.leaves(cap)


def test_a_fresh_tree_pushes_one_and_the_run_wraps(L):
    tree, c = np.zeros(16, np.float32), cur(pos=3)
    RP.push(L, tree, c, 4, 5)                                            # slots 3, 4, 0, 1
    assert tree[8:].tolist() == [1, 1, 0, 1, 1, 0, 0, 0] and tree[1] == 4 and tree[0] == 0 and c.tolist() == [3, 0, 0, 0]
    assert tree[1:8].tolist() == [4, 3, 1, 2, 1, 1, 0]
    tree[0] = np.float32(2.0 ** -41)                                     # below MIN reads as 1.0 too
    RP.push(L, tree, cur(pos=2), 1, 5)
    assert tree[10] == 1 and tree[1] == 5 and tree[0] == np.float32(2.0 ** -41)
    tree[0] = 6.5                                                        # later pushes hand out the largest priority seen
    RP.push(L, tree, cur(pos=4), 2, 5)
    assert tree[8:13].tolist() == [6.5, 1, 1, 1, 6.5] and tree[1] == 16 and tree[0] == 6.5


def test_known_answers_on_four_slots(L):
    tree, c = np.zeros(8, np.float32), cur(size=4)
    RP.update(L, tree, c, [0, 1, 2, 3], [1, 2, 3, 4], 4)
    assert tree.tolist() == [4, 10, 3, 7, 1, 2, 3, 4]
    # m < 1 -> slot 0; [1, 3) -> 1; [3, 6) -> 2; [6, 10] -> 3 (m == total still lands on the last slot)
    for m, want in ((0, 0), (0.99, 0), (1, 1), (2.5, 1), (2.999, 1), (3, 2), (5.9, 2), (6, 3), (9.99, 3), (10, 3), (11, 3)):
        assert L.prio_descend(4, tree.ctypes.data, m) == want, m
    # the r > 0 guard: with slots 2, 3 empty, a mass at or beyond the total stays on the last positive leaf
    t2, c2 = np.zeros(8, np.float32), cur(size=2)
    RP.update(L, t2, c2, [0, 1], [1, 2], 4)
    assert t2.tolist() == [2, 3, 3, 0, 1, 2, 0, 0]
    assert [L.prio_descend(4, t2.ctypes.data, m) for m in (0, 1, 2.9, 3, 3.5)] == [0, 1, 1, 1, 1]
    # one draw per quarter of the mass: element b aims into [b, b + 1) * total / B
    for b in range(4):
        m = L.prio_mass(99, 0, b, 4, 10.0)
        assert 2.5 * b <= m <= 2.5 * (b + 1)
    assert L.prio_mass(99, 0, 1, 4, 10.0) != L.prio_mass(99, 1, 1, 4, 10.0) != L.prio_mass(98, 1, 1, 4, 10.0)


def test_clamp(L):
    want = [MIN, MIN, MIN, MIN, MIN, MIN, MAX, MAX, MIN, MAX, 1.0, np.float32(0.3), 7.5]
    got = [L.prio_clamp(float(p)) for p in RP.ODD_PRIORITIES]
    assert bits(np.array(got, np.float32)).tolist() == bits(np.array(want, np.float32)).tolist()
    n = len(want)
    tree, c = np.zeros(2 * 16, np.float32), cur(size=n)
    RP.update(L, tree, c, np.arange(n), RP.ODD_PRIORITIES, n)
    assert bits(tree[16:16 + n]).tolist() == bits(np.array(want, np.float32)).tolist() and tree[0] == MAX


def test_duplicates_take_the_max_and_invalid_indices_are_ignored(L):
    cap = 10
    tree, c = RP.random_tree(np.random.default_rng(1), cap, 6, -3, 3, top=9.0), cur(size=6)
    before = tree.copy()
    idx = [2, -1, 2, 6, 10, 2 ** 31 - 1, 2, -5, 4]                    # 6 = size, 10 = capacity
    pri = [0.5, 99, 3.0, 98, 97, 96, 2.0, 95, np.nan]
    RP.update(L, tree, c, idx, pri, cap)
    assert tree[16 + 2] == 3.0 and tree[16 + 4] == MIN and tree[0] == 9.0
    untouched = [0, 1, 3, 5, 6, 7, 8, 9]
    assert np.array_equal(bits(tree[16:][untouched]), bits(before[16:][untouched]))
    assert np.array_equal(bits(tree), bits(RP.rebuilt(tree)))
    RP.update(L, tree, c, [1, 1], [20.0, 10.0], cap)                   # the running max rises with a valid element only
    assert tree[17] == 20.0 and tree[0] == 20.0
    RP.update(L, tree, c, [7], [1000.0], cap)
    assert tree[0] == 20.0 and tree[16 + 7] == 0
    fresh = np.zeros(32, np.float32)
    RP.update(L, fresh, c, [-1], [5.0], cap)                           # tree[0] is written as read: 1.0 from a fresh tree
    assert fresh[0] == 1.0 and not fresh[1:].any()
    RP.update(L, fresh, c, [3], [0.25], cap)
    assert fresh[0] == 1.0 and fresh[19] == 0.25 and fresh[1] == 0.25


# ------------------------------------------------------------------------------------------ the sampling rule
@pytest.mark.parametrize('all_min', [False, True])
@pytest.mark.parametrize('cap', [5, 64, 100, 311, 1000, 4097])
def test_sampled_indices_are_held_positive_and_nondecreasing(L, cap, all_min):
    rng = np.random.default_rng(cap + all_min)
    for size in sorted({s for s in (1, 7, 37, 200, cap) if s <= cap}):
        tree = RP.random_tree(rng, cap, size, -40, -40 if all_min else 40)
        if all_min:
            assert (tree[RP.leaves(cap):][:size] == MIN).all()
        for B in (1, 64, 333):
            idx = RP.indices(L, tree, cap, B, seed=7, samples=size)
            assert idx.min() >= 0 and idx.max() < size, (cap, size, B)
            assert (tree[RP.leaves(cap) + idx] > 0).all() and (np.diff(idx) >= 0).all(), (cap, size, B)


def test_sampling_is_proportional_to_priority(L):
    """64 slots with priorities 1..64, 16 calls of B = 4096: chi-square of the counts against p / sum(p) * 65536 below the
    1 - 1e-6 quantile at 63 degrees of freedom (stratified draws sit far below it; a uniform or sqrt(p) sampler far above)"""
    cap, B, calls = 64, 4096, 16
    ring = RR.Ring(cap, 1, 1)
    ring.cursor[:] = (0, cap, 1, 0)
    tree = np.zeros(128, np.float32)
    RP.update(L, tree, ring.cursor, np.arange(cap), np.arange(1, cap + 1), cap)
    assert tree[1] == 2080 and tree[0] == 64
    counts = np.zeros(cap)
    for _ in range(calls):
        counts += np.bincount(RP.sample(L, ring, tree, B, seed=2024)['index'], minlength=cap)
    assert ring.cursor[3] == calls and counts.sum() == B * calls
    expect = np.arange(1, cap + 1) / 2080.0 * B * calls
    stat = float(((counts - expect) ** 2 / expect).sum())
    uniform = float(((B * calls / cap - expect) ** 2 / expect).sum())
    print(f'chi2 = {stat:.2f} (limit {CHI2_63:.1f}; a uniform sampler would give {uniform:.0f})')
    assert stat < CHI2_63 < uniform


def test_restated_sample_fields_and_the_empty_cases(L):
    rng = np.random.default_rng(3)
    cap, D, AW, B, seed = 50, 5, 3, 133, 0x0123456789ABCDEF
    ring = RR.Ring(cap, D, AW)
    for k in ('obs', 'next_obs', 'action'):
        getattr(ring, k)[:] = rng.integers(0, 2 ** 32, getattr(ring, k).shape, dtype=np.uint64).astype(np.uint32)
    ring.reward[:], ring.discount[:] = rng.standard_normal(cap), rng.standard_normal(cap)
    ring.cursor[:] = (7, 31, 2, 0)
    tree = RP.random_tree(rng, cap, 31, -5, 5)
    a, b = RP.sample(L, ring, tree, B, seed), RP.sample(L, ring, tree, B, seed)
    assert ring.cursor.tolist() == [7, 31, 2, 2] and not np.array_equal(a['index'], b['index'])
    for n, got in ((0, a), (1, b)):
        idx = RP.indices(L, tree, cap, B, seed, n)
        assert np.array_equal(got['index'], idx) and bits(got['total'])[0] == bits(tree[1:2])[0]
        assert np.array_equal(bits(got['priority']), bits(tree[64 + idx]))
        for k in RR.RING_FIELDS:
            assert np.array_equal(bits(got[k]), bits(getattr(ring, k)[idx])), k
    for size, t in ((0, tree), (31, np.zeros_like(tree))):              # nothing held | nothing to draw from
        ring.cursor[1] = size
        z = RP.sample(L, ring, t, 9, seed)
        assert (z['index'] == -1).all() and not any(bits(z[k]).any() for k in RP.BATCH_FIELDS if k != 'index')


# ------------------------------------------------------------------------------------------ PrioritizedReplay argument checks
def cpu_buffer(**kw):
    from soccer2d_amd.replay import PrioritizedReplay
    return PrioritizedReplay(**{**dict(capacity=64, obs_dim=4, device='cpu'), **kw})


@pytest.mark.parametrize('kw', [dict(capacity=0), dict(capacity=2 ** 30 + 1), dict(capacity=True), dict(obs_dim=0), dict(action_words=9),
                                dict(n_step=0), dict(gamma=float('nan')), dict(action_dtype=torch.int64), dict(seed=-1)])
def test_constructor_rejects(kw):
    with pytest.raises(ValueError, match='PrioritizedReplay|DeviceReplay'):
        cpu_buffer(**kw)


def test_the_buffer_owns_a_zero_tree_of_tree_words():
    from soccer2d_amd.replay import DeviceReplay
    for cap, words in ((1, 2), (64, 128), (65, 256), (100, 256)):
        rb = cpu_buffer(capacity=cap)
        assert isinstance(rb, DeviceReplay) and rb.tree.dtype == torch.float32 and tuple(rb.tree.shape) == (words,) and not rb.tree.any()
    assert (rb.total, rb.max_priority) == (0.0, 1.0)
    rb.tree[0], rb.tree[1] = 3.0, 7.0
    assert (rb.total, rb.max_priority) == (7.0, 3.0)
    rb.cursor[1] = 5
    rb.clear()
    assert not rb.tree.any() and rb.cursor.tolist() == [0, 0, 0, 0]


def test_calls_reject_before_any_library_call():
    from test_replay_host import cpu_record
    rb = cpu_buffer()
    rec, first = cpu_record()
    big, big_first = cpu_record(T=9, N=8)
    with pytest.raises(ValueError, match='capacity'):
        rb.push(big, big_first)
    with pytest.raises(ValueError, match='terminal_obs'):
        rb.push({k: v for k, v in rec.items() if k != 'terminal_obs'}, first)
    for bad in (0, 2 ** 24 + 1, 1.5):
        with pytest.raises(ValueError, match='batch'):
            rb.sample(bad)
    out = rb.alloc_batch(16)
    assert set(out) == {'obs', 'next_obs', 'action', 'reward', 'discount', 'index', 'priority', 'total'}
    assert tuple(out['priority'].shape) == (16,) and tuple(out['total'].shape) == (1,) and out['total'].dtype == torch.float32
    with pytest.raises(ValueError, match='priority'):
        rb.sample(16, out={k: v for k, v in out.items() if k != 'priority'})
    with pytest.raises(ValueError, match='total'):
        rb.sample(16, out={**out, 'total': torch.zeros(2)})
    idx, pri = torch.zeros(16, dtype=torch.int32), torch.ones(16)
    for i, p, text in ((idx.long(), pri, 'index'), (idx, pri.double(), 'priority'), (idx, pri[:8], 'priority'), (idx[::2], pri[:8], 'index'),
                       (idx[:0], pri[:0], 'index'), (idx.reshape(4, 4), pri, 'index'), ([0] * 16, pri, 'index')):
        with pytest.raises(ValueError, match=text):
            rb.update_priorities(i, p)
    for beta in (-0.1, float('nan'), None):
        with pytest.raises(ValueError, match='beta'):
            rb.weights(out, beta)
    with pytest.raises(ValueError, match='priority'):
        rb.weights({'index': idx}, 0.4)
    # well-formed calls on a CPU buffer are refused too: there is no CPU path
    for call in (lambda: rb.push(rec, first), lambda: rb.sample(16), lambda: rb.update_priorities(idx, pri)):
        with pytest.raises(ValueError, match='GPU'):
            call()
    assert not rb.tree.any() and rb.cursor.tolist() == [0, 0, 0, 0]


def test_weights_are_pure_torch():
    rb = cpu_buffer(capacity=8)
    rb.cursor[1] = 100                                                  # read as min(size, capacity) = 8
    batch = {'index': torch.tensor([0, 3, -1, 5], dtype=torch.int32), 'priority': torch.tensor([1.0, 4.0, 0.0, 2.0]),
             'total': torch.tensor([16.0])}
    w = rb.weights(batch, 0.5)                                          # (8 p / 16) ** -0.5 = sqrt(2 / p), over the largest
    assert torch.allclose(w, torch.tensor([1.0, 0.5, 0.0, 0.5 ** 0.5])) and w.dtype == torch.float32
    assert rb.weights(batch, 0).tolist() == [1.0, 1.0, 0.0, 1.0]
    empty = {'index': torch.full((4,), -1, dtype=torch.int32), 'priority': torch.zeros(4), 'total': torch.zeros(1)}
    assert rb.weights(empty, 0.4).tolist() == [0.0, 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------ header / mirror / library
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    return _capi.load_library()


def test_prio_entry_points_declared_bound_and_exported(lib):
    from soccer2d_amd import _capi
    names = declared_functions(HDR)
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    for n in NEW:
        assert n in names and n in protos and hasattr(lib, n), n
    assert [len(protos[n][2]) for n in NEW] == [1, 5, 7, 16]
    hdr = open(HDR).read()
    assert _capi.S2D_ABI_VERSION == 4 and '#define S2D_ABI_VERSION 4' in hdr
    assert '#define S2D_REPLAY_PRIO_STREAM 12' in hdr and '#define S2D_PRIO_MIN 0x1p-40f' in hdr and '#define S2D_PRIO_MAX 0x1p+40f' in hdr


def test_tree_words_needs_no_gpu(lib, L):
    for cap in (1, 2, 3, 4, 5, 64, 65, 100, 4096, 4097, 2 ** 22, 2 ** 30 - 1, 2 ** 30):
        assert lib.s2d_replay_tree_words(cap) == 2 * L.prio_leaves(cap) == 2 * RP.leaves(cap), cap
    assert [lib.s2d_replay_tree_words(c) for c in (0, -1, 2 ** 30 + 1, 2 ** 62)] == [0, 0, 0, 0]
    assert lib.s2d_replay_tree_words(2 ** 30) == 2 ** 31


def test_entry_points_reject_without_a_gpu(lib):
    """argument checks come before any HIP call: every pointer below is a made-up address that is never dereferenced"""
    from soccer2d_amd import _capi
    tree, cursor, st = 0x800000, 0x60000, None                          # capacity 100: the tree is 256 floats = 1 KiB

    def check(rc, text, name, kw):
        assert rc == _capi.S2D_EINVAL, kw
        assert text in lib.s2d_last_error() and name in lib.s2d_last_error(), (kw, lib.s2d_last_error())

    def push(n=10, cap=100, tree=tree, cur=cursor):
        return lib.s2d_replay_prio_push(n, cap, tree, cur, st)

    for kw, text in ((dict(n=0), b'n must'), (dict(n=101), b'n must'), (dict(cap=0), b'capacity'), (dict(cap=2 ** 30 + 1, n=1), b'capacity'),
                     (dict(tree=None), b'non-NULL'), (dict(cur=None), b'non-NULL'), (dict(tree=tree + 4), b'8-byte'),
                     (dict(cur=cursor + 4), b'8-byte'), (dict(cur=tree + 1016), b'overlap'), (dict(tree=cursor - 1016), b'overlap')):
        check(push(**kw), text, b's2d_replay_prio_push', kw)

    idx, pri = 0x100000, 0x200000

    def update(B=32, cap=100, tree=tree, cur=cursor, idx=idx, pri=pri):
        return lib.s2d_replay_prio_update(B, cap, tree, cur, idx, pri, st)

    for kw, text in ((dict(B=0), b'batch'), (dict(B=2 ** 24 + 1), b'batch'), (dict(cap=0), b'capacity'), (dict(cap=2 ** 31), b'capacity'),
                     (dict(tree=None), b'non-NULL'), (dict(idx=None), b'non-NULL'), (dict(pri=None), b'non-NULL'),
                     (dict(tree=tree + 4), b'8-byte'), (dict(cur=cursor + 4), b'8-byte'), (dict(idx=idx + 2), b'4-byte'),
                     (dict(pri=pri + 1), b'4-byte'), (dict(idx=tree + 512), b'overlap'), (dict(pri=tree - 64), b'overlap'),
                     (dict(cur=tree + 8), b'overlap')):
        check(update(**kw), text, b's2d_replay_prio_update', kw)

    ring = _capi.S2DReplayRing(100, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000)
    batch = (0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x780000)

    def sample(B=32, D=4, AW=1, ring=ring, tree=tree, cur=cursor, batch=batch):
        return lib.s2d_replay_sample_prio(B, D, AW, C.byref(ring) if ring is not None else None, tree, cur, 1, *batch, st)

    def ring_cap(cap):
        return _capi.S2DReplayRing(cap, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000)

    for kw, text in ((dict(B=0), b'batch'), (dict(B=2 ** 24 + 1), b'batch'), (dict(D=1025), b'obs_dim'), (dict(AW=9), b'action_words'),
                     (dict(ring=None), b'ring'), (dict(ring=ring_cap(0)), b'capacity'), (dict(ring=ring_cap(2 ** 30 + 1)), b'capacity'),
                     (dict(tree=None), b'non-NULL'), (dict(cur=None), b'non-NULL'), (dict(tree=tree + 4), b'8-byte'),
                     (dict(cur=cursor + 4), b'8-byte'), (dict(batch=batch[:6] + (None, batch[7])), b'non-NULL'),
                     (dict(batch=batch[:7] + (None,)), b'non-NULL'), (dict(batch=(0x100008,) + batch[1:]), b'16-byte'),
                     (dict(batch=batch[:6] + (0x700002, batch[7])), b'4-byte'), (dict(batch=batch[:7] + (0x780001,)), b'4-byte'),
                     (dict(batch=batch[:6] + (tree + 1020, batch[7])), b'overlap'),      # priority on the tree's last word
                     (dict(batch=batch[:7] + (tree,)), b'overlap'),                      # total on tree[0]
                     (dict(batch=batch[:7] + (0x700000 + 64,)), b'overlap'),             # total inside priority
                     (dict(batch=batch[:5] + (cursor,) + batch[6:]), b'overlap'),
                     (dict(tree=0x40000 - 1016), b'overlap'),                            # the tree's tail on the ring's reward
                     (dict(tree=cursor - 8), b'overlap')):
        check(sample(**kw), text, b's2d_replay_sample_prio', kw)
