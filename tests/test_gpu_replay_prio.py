"""Prioritized replay on the GPU (s2d_replay_prio_push / s2d_replay_prio_update / s2d_replay_sample_prio, raw and through
soccer2d_amd.replay.PrioritizedReplay): the whole tree after a push mark or an update, and every field of a sampled batch,
against the host restatement (tests/replay_prio_ref.c) over every tier edge of the repair, the wave edges, duplicates, invalid
indices and the clamp; the empty cases; proportionality; a closed loop eagerly and in one captured graph; rejections.  Every
comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest

import replay as RR
import replay_prio as RP

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
SENTINEL = 0xA5A5A5A5
GAMMA = 0.97
INT32_MAX = 2 ** 31 - 1
CHI2_63 = 131.3697020515818          # scipy.stats.chi2.ppf(1 - 1e-6, 63), the convention of test_gpu_distributions.py


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return RP.build(tmp_path_factory.mktemp('replay_prio_ref'))


@pytest.fixture(scope='module')
def LR(tmp_path_factory):
    return RR.build(tmp_path_factory.mktemp('replay_ref'))


@pytest.fixture(scope='module')
def lib():
    from soccer2d_amd import _capi
    return _capi.load_library()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def words_of(t):
    return t.view(torch.int32)


def dev_rec(rec):
    return {k: torch.from_numpy(v).to(DEV) for k, v in rec.items()}


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def twin(capacity, D=1, AW=1, float_action=False, n_step=1, seed=0, fill=SENTINEL, cursor=(0, 0, 0, 0), tree=None):
    """a PrioritizedReplay and a host ring in the same state: every ring word the sentinel, the same cursor, the given tree"""
    from soccer2d_amd.replay import PrioritizedReplay
    rb = PrioritizedReplay(capacity, D, action_words=AW, action_dtype=torch.float32 if float_action else torch.int32, device=DEV,
                           n_step=n_step, gamma=GAMMA, seed=seed)
    ring = RR.Ring(capacity, D, AW, fill=fill)
    for k in RR.RING_FIELDS:
        words_of(getattr(rb, k)).fill_(int(np.uint32(fill).view(np.int32)))
    ring.cursor[:] = cursor
    rb.cursor.copy_(torch.tensor(cursor, dtype=torch.int64))
    assert tuple(rb.tree.shape) == (2 * RP.leaves(capacity),) and not rb.tree.any()
    if tree is not None:
        rb.tree.copy_(torch.from_numpy(tree))
    return rb, ring


def load_ring(rb, ring):
    for k in RR.RING_FIELDS:
        words_of(getattr(rb, k)).copy_(torch.from_numpy(bits(getattr(ring, k)).view(np.int32)))
    rb.cursor.copy_(torch.from_numpy(ring.cursor.astype(np.int64)))


def random_ring(rng, cap, D, AW, cursor):
    ring = RR.Ring(cap, D, AW)
    for k in RR.RING_FIELDS:
        a = bits(getattr(ring, k))
        a[...] = rng.integers(0, 2 ** 32, a.shape, dtype=np.uint64).astype(np.uint32)
    ring.cursor[:] = cursor
    return ring


def same_tree(rb, tree, what):
    torch.cuda.synchronize()
    got = bits(rb.tree.cpu().numpy())
    bad = np.flatnonzero(got != bits(tree))
    assert bad.size == 0, f'{what}: the tree differs in {bad.size} nodes, first {bad[:8]}: {got[bad[:8]]} != {bits(tree)[bad[:8]]}'


def same_ring(rb, ring, what):
    torch.cuda.synchronize()
    for k in RR.RING_FIELDS:
        got, want = bits(getattr(rb, k).cpu().numpy()).reshape(ring.capacity, -1), bits(getattr(ring, k)).reshape(ring.capacity, -1)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f'{what}: {k} differs in {bad.size} slots, first {bad[:5]}'
    assert rb.cursor.cpu().tolist() == ring.cursor.tolist(), what


def same_batch(got, want, what):
    torch.cuda.synchronize()
    for k in RP.BATCH_FIELDS:
        n = want[k].shape[0]
        g, w = bits(got[k].cpu().numpy()).reshape(n, -1), bits(want[k]).reshape(n, -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, f'{what}: {k} differs in {bad.size} elements, first {bad[:5]}'


# ------------------------------------------------------------------------------------------ prio_push
def push_runs(cap):
    """(pos, n): one slot, the whole ring from a middle position, a run inside one 64-leaf group, a run that wraps at the capacity"""
    g = (cap // 2) // 64 * 64                               # the first leaf of a middle group
    runs = [(cap // 3, 1), (cap // 2, cap), (g + 1, min(7, cap - g - 1)), (cap - 1, min(cap, 3)), (cap - min(cap, 70), min(cap, 70 + 5))]
    return sorted({(p, n) for p, n in runs if 0 <= p < cap and 1 <= n <= cap})


@pytest.mark.parametrize('cap', [1, 2, 3, 64, 65, 100, 4096, 4097])      # P = 1, 2, 4, 64, 128, 128, 4096, 8192
def test_prio_push_equals_restatement_the_whole_tree(L, lib, cap):
    rng = np.random.default_rng(cap)
    for k, (pos, n) in enumerate(push_runs(cap)):
        size = cap if k % 2 else max(1, cap // 2)
        start = RP.random_tree(rng, cap, size, -10, 10, top=(0.0, 2.0 ** -41, 37.5, 2.0 ** 40)[k % 4])
        rb, ring = twin(cap, cursor=(pos + 3 * cap, size, 4, 9) if k == 0 else (pos, size, 4, 9), tree=start)
        want = start.copy()
        assert lib.s2d_replay_prio_push(n, cap, ptr(rb.tree), ptr(rb.cursor), stream()) == 0, lib.s2d_last_error()
        RP.push(L, want, ring.cursor, n, cap)
        same_tree(rb, want, f'cap={cap} pos={pos} n={n}')
        same_ring(rb, ring, f'cap={cap} pos={pos} n={n}: the ring and the cursor are untouched')
        assert bits(want[:1])[0] == bits(start[:1])[0] and want[RP.leaves(cap) + pos] == (start[0] if start[0] >= RP.PRIO_MIN else 1.0)


# ------------------------------------------------------------------------------------------ prio_update
def update_indices(rng, kind, B, size):
    if kind == 'range5':
        base = int(rng.integers(0, max(1, size - 5)))
        return rng.integers(base, min(size, base + 5), B)
    if kind == 'identical':
        return np.full(B, int(rng.integers(0, size)))
    if B <= size:                                                       # 'distinct'
        return rng.permutation(size)[:B]
    return rng.permutation(B) % size                                    # more elements than slots: as evenly spread as they can be


@pytest.mark.parametrize('kind', ['range5', 'identical', 'distinct'])
@pytest.mark.parametrize('cap,size', [(100, 70), (4097, 4097)])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 1000])
def test_prio_update_equals_restatement_the_whole_tree(L, lib, B, cap, size, kind):
    rng = np.random.default_rng(B * 10 + cap + len(kind))
    start = RP.random_tree(rng, cap, size, -6, 6, top=(0.0 if B % 2 else 3.0))
    idx = update_indices(rng, kind, B, size).astype(np.int64)
    pri = np.where(rng.random(B) < 0.5, rng.choice(RP.ODD_PRIORITIES, B), np.exp2(rng.uniform(-45, 45, B))).astype(np.float32)
    if B > 1:                                                           # invalid entries among the valid ones, with loud priorities
        bad = rng.random(B) < 0.15
        idx[bad] = rng.choice([-1, size, cap, INT32_MAX, -2 ** 31], int(bad.sum()))
    idx = idx.astype(np.int32)
    rb, ring = twin(cap, cursor=(5, size if size < cap else cap + 1000, 2, 1), tree=start)
    want = start.copy()
    d_idx, d_pri = torch.from_numpy(idx).to(DEV), torch.from_numpy(pri).to(DEV)
    assert lib.s2d_replay_prio_update(B, cap, ptr(rb.tree), ptr(rb.cursor), ptr(d_idx), ptr(d_pri), stream()) == 0, lib.s2d_last_error()
    RP.update(L, want, ring.cursor, idx, pri, cap)
    same_tree(rb, want, f'B={B} cap={cap} {kind}')
    same_ring(rb, ring, 'the ring and the cursor are untouched')
    assert np.array_equal(d_idx.cpu().numpy(), idx) and np.array_equal(bits(d_pri.cpu().numpy()), bits(pri))
    assert want[0] >= 1 and np.array_equal(bits(want), bits(RP.rebuilt(want)))


def test_update_through_the_class_clamps_and_takes_the_max(L):
    n = len(RP.ODD_PRIORITIES)
    rb, ring = twin(40, cursor=(0, n + 2, 1, 0))
    idx = np.concatenate([np.arange(n), [n, n, n + 1, -1]]).astype(np.int32)
    pri = np.concatenate([RP.ODD_PRIORITIES, [2.0, 5.0, np.nan, 9.0]]).astype(np.float32)
    rb.update_priorities(torch.from_numpy(idx).to(DEV), torch.from_numpy(pri).to(DEV))
    want = np.zeros(128, np.float32)
    RP.update(L, want, ring.cursor, idx, pri, 40)
    same_tree(rb, want, 'the clamp list')
    assert want[64 + n] == 5.0 and want[64 + n + 1] == RP.PRIO_MIN and want[0] == RP.PRIO_MAX
    assert rb.max_priority == float(RP.PRIO_MAX) and rb.total == float(want[1])


def test_a_tree_of_four_tiers(L, lib):
    """capacity 2^18 + 1: P = 2^19, repaired in tiers of 6 + 6 + 6 + 1 levels; a push mark that wraps, then an update"""
    cap = 2 ** 18 + 1
    rng = np.random.default_rng(19)
    start = RP.random_tree(rng, cap, cap, -20, 20)
    rb, ring = twin(cap, cursor=(cap - 1000, cap, 7, 0), tree=start)
    want = start.copy()
    assert lib.s2d_replay_prio_push(5000, cap, ptr(rb.tree), ptr(rb.cursor), stream()) == 0, lib.s2d_last_error()
    RP.push(L, want, ring.cursor, 5000, cap)
    same_tree(rb, want, 'push mark')
    idx = rng.integers(0, cap, 1000).astype(np.int32)
    idx[::7] = idx[3]
    pri = np.exp2(rng.uniform(-45, 45, 1000)).astype(np.float32)
    rb.update_priorities(torch.from_numpy(idx).to(DEV), torch.from_numpy(pri).to(DEV))
    RP.update(L, want, ring.cursor, idx, pri, cap)
    same_tree(rb, want, 'update')
    got = rb.sample(300)
    same_batch(got, RP.sample(L, ring, want, 300, 0), 'sample')


# ------------------------------------------------------------------------------------------ sample_prio
@pytest.mark.parametrize('D,AW', [(10, 1), (4, 4), (224, 1)])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 1000])
def test_sample_prio_equals_restatement(L, B, D, AW):
    rng = np.random.default_rng(B + D)
    cap, seed = 311, 0xFEDCBA9876543210
    for size in (1, 7, cap):
        for all_min in (False, True):
            what = f'B={B} D={D} size={size} all_min={all_min}'
            ring = random_ring(rng, cap, D, AW, (11, size, 3, 5))
            tree = RP.random_tree(rng, cap, size, -40, -40 if all_min else 40)
            rb, _ = twin(cap, D, AW, AW == 4, seed=seed, tree=tree)
            load_ring(rb, ring)
            first, second = rb.sample(B), rb.sample(B)
            w1, w2 = RP.sample(L, ring, tree, B, seed), RP.sample(L, ring, tree, B, seed)
            same_batch(first, w1, what + ' call 0')
            same_batch(second, w2, what + ' call 1')
            same_ring(rb, ring, what + ': sampling changes only the sample counter')
            same_tree(rb, tree, what)
            assert ring.cursor.tolist() == [11, size, 3, 7] and 0 <= w1['index'].min() and w1['index'].max() < size
            assert (np.diff(w1['index']) >= 0).all() and (w1['priority'] > 0).all() and w1['total'][0] == tree[1]
            if all_min and size == cap and B > 1:
                assert not np.array_equal(w1['index'], w2['index'])
                assert not torch.equal(first['index'], second['index'])


def test_one_slot_is_the_whole_tree(L):
    """capacity 1: P = 1, the total is the leaf, no descent"""
    ring = random_ring(np.random.default_rng(1), 1, 3, 2, (0, 1, 1, 0))
    tree = np.array([2.5, 2.5], np.float32)
    rb, _ = twin(1, 3, 2, tree=tree)
    load_ring(rb, ring)
    got = rb.sample(70)
    same_batch(got, RP.sample(L, ring, tree, 70, 0), 'capacity 1')
    assert (got['index'] == 0).all() and (got['priority'] == 2.5).all()


@pytest.mark.parametrize('size,zero_tree', [(0, False), (40, True), (0, True)])
def test_an_empty_buffer_or_an_empty_tree_gives_the_zero_batch(L, size, zero_tree):
    rng = np.random.default_rng(6)
    ring = random_ring(rng, 100, 10, 2, (0, size, 0, 0))
    tree = np.zeros(256, np.float32) if zero_tree else RP.random_tree(rng, 100, 30)
    rb, _ = twin(100, 10, 2, tree=tree)
    load_ring(rb, ring)
    out = rb.alloc_batch(130)
    for k in RP.BATCH_FIELDS:
        words_of(out[k]).fill_(0x1234567)
    got = rb.sample(130, out=out)
    assert got is out
    same_batch(got, RP.sample(L, ring, tree, 130, 0), 'empty')
    assert (out['index'] == -1).all() and not any(words_of(out[k]).any() for k in RP.BATCH_FIELDS if k != 'index')
    assert rb.cursor.cpu().tolist() == [0, size, 0, 1]
    assert rb.weights(out, 0.4).cpu().tolist() == [0.0] * 130
    rb.update_priorities(out['index'], torch.full((130,), 50.0, device=DEV))     # the -1s of an empty batch are ignored
    want = tree.copy()
    want[0] = want[0] if want[0] >= RP.PRIO_MIN else 1.0                # written as read
    same_tree(rb, want, 'update with an empty batch')


def test_sampling_is_proportional_to_priority(L):
    """64 slots with priorities 1..64, 16 calls of B = 4096: chi-square of the counts against p / sum(p) * 65536 below the
    1 - 1e-6 quantile at 63 degrees of freedom; the indices of two of the calls also equal the restatement's"""
    cap, B, calls, seed = 64, 4096, 16, 2024
    rb, ring = twin(cap, seed=seed, cursor=(0, cap, 1, 0))
    rb.update_priorities(torch.arange(cap, dtype=torch.int32, device=DEV), torch.arange(1, cap + 1, dtype=torch.float32, device=DEV))
    tree = np.zeros(128, np.float32)
    RP.update(L, tree, ring.cursor, np.arange(cap), np.arange(1, cap + 1), cap)
    same_tree(rb, tree, 'priorities 1..64')
    assert (rb.total, rb.max_priority) == (2080.0, 64.0)
    counts, out = np.zeros(cap), rb.alloc_batch(B)
    for n in range(calls):
        idx = rb.sample(B, out=out)['index'].cpu().numpy()
        if n in (0, calls - 1):
            assert np.array_equal(idx, RP.indices(L, tree, cap, B, seed, n)), n
        counts += np.bincount(idx, minlength=cap)
    expect = np.arange(1, cap + 1) / 2080.0 * B * calls
    stat = float(((counts - expect) ** 2 / expect).sum())
    print(f'chi2 = {stat:.2f} (limit {CHI2_63:.1f})')
    assert counts.sum() == B * calls and stat < CHI2_63
    w = rb.weights(out, 1.0).cpu().numpy()                               # beta = 1: weight * priority is one constant
    pri = out['priority'].cpu().numpy()
    assert np.allclose(w * pri, pri.min(), rtol=1e-5) and w.max() == 1.0


# ------------------------------------------------------------------------------------------ closed loop, eager and captured
def new_priority(reward, out=None):
    """the priorities the closed loop derives from a batch: |reward| + 0.5, two exact-rounded fp32 operations on either side"""
    if torch.is_tensor(reward):
        out = torch.abs(reward, out=out)
        return out.add_(0.5)
    return (np.abs(reward) + np.float32(0.5)).astype(np.float32)


def test_closed_loop_eagerly_and_in_one_captured_graph(L, LR):
    rng = np.random.default_rng(9)
    T, N, D, AW, B, cap = 5, 130, 10, 1, 200, 1500                      # the third push wraps (3 * 650 > 1500)
    recs = [RR.synthetic_record(rng, T, N, D, AW) for _ in range(4)]
    eager, ring = twin(cap, D, AW, n_step=3, seed=77)
    tree = np.zeros(2 * RP.leaves(cap), np.float32)
    eager_batches = []
    for n in range(3):
        h_rec, h_first = recs[n]
        eager.push(dev_rec(h_rec), torch.from_numpy(h_first).to(DEV))
        got = eager.sample(B)
        eager.update_priorities(got['index'], new_priority(got['reward']))
        RP.push(L, tree, ring.cursor, T * N, cap)
        RR.push(LR, ring, h_rec, h_first, 3, GAMMA)
        want = RP.sample(L, ring, tree, B, 77)
        same_batch(got, want, f'round {n}')
        RP.update(L, tree, ring.cursor, want['index'], new_priority(want['reward']), cap)
        same_ring(eager, ring, f'round {n}')
        same_tree(eager, tree, f'round {n}')
        assert ring.cursor.tolist() == [(n + 1) * T * N % cap, min((n + 1) * T * N, cap), n + 1, n + 1]
        eager_batches.append({k: v.clone() for k, v in got.items()})
    assert len(np.unique(tree[RP.leaves(cap):][:cap])) > 100             # the priorities did spread

    rb, _ = twin(cap, D, AW, n_step=3, seed=77)
    rec, first = dev_rec(recs[3][0]), torch.from_numpy(recs[3][1]).to(DEV)
    batch, pri = rb.alloc_batch(B), torch.empty(B, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # a warm-up outside the capture, on a buffer of its own
        warm, _ = twin(cap, D, AW, n_step=3, seed=77)
        warm.push(rec, first)
        wb = warm.sample(B)
        warm.update_priorities(wb['index'], new_priority(wb['reward'], out=torch.empty(B, device=DEV)))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                       # prio_push, push, sample_prio, prio_update: a linear chain
        rb.push(rec, first)
        rb.sample(B, out=batch)
        rb.update_priorities(batch['index'], new_priority(batch['reward'], out=pri))
    torch.cuda.synchronize()
    assert rb.cursor.cpu().tolist() == [0, 0, 0, 0] and not rb.tree.any()   # capturing ran nothing
    for n in range(3):
        for k, v in recs[n][0].items():
            rec[k].copy_(torch.from_numpy(v))
        first.copy_(torch.from_numpy(recs[n][1]))
        graph.replay()
        torch.cuda.synchronize()
        for k in RP.BATCH_FIELDS:
            assert torch.equal(words_of(batch[k]), words_of(eager_batches[n][k])), (n, k)
    for k in RR.RING_FIELDS + ('tree',):
        assert torch.equal(words_of(getattr(rb, k)), words_of(getattr(eager, k))), k
    assert rb.cursor.cpu().tolist() == eager.cursor.cpu().tolist() == ring.cursor.tolist()


# ------------------------------------------------------------------------------------------ rejections
def test_rejections_return_einval_with_text_and_launch_nothing(lib):
    from soccer2d_amd import _capi
    rng = np.random.default_rng(10)
    cap, D, B = 500, 4, 50
    start = RP.random_tree(rng, cap, 300)
    rb, ring = twin(cap, D, cursor=(3, 300, 1, 0), tree=start)
    st, tree, cur = stream(), rb.tree.data_ptr(), rb.cursor.data_ptr()
    idx, pri = torch.zeros(B, dtype=torch.int32, device=DEV), torch.ones(B, device=DEV)
    out = rb.alloc_batch(B)
    for k in RP.BATCH_FIELDS:
        words_of(out[k]).fill_(0x7654321)

    def refused(rc, text, name, kw):
        assert rc == _capi.S2D_EINVAL, kw
        assert text in lib.s2d_last_error() and name in lib.s2d_last_error(), (kw, lib.s2d_last_error())

    def push(n=10, cap=cap, tree=tree, cur=cur):
        return lib.s2d_replay_prio_push(n, cap, tree, cur, st)

    for kw, text in [(dict(n=0), b'n must'), (dict(n=cap + 1), b'n must'), (dict(cap=0), b'capacity'), (dict(tree=None), b'non-NULL'),
                     (dict(cur=None), b'non-NULL'), (dict(tree=tree + 4), b'8-byte'), (dict(cur=cur + 4), b'8-byte'),
                     (dict(cur=tree + 64), b'overlap')]:
        refused(push(**kw), text, b's2d_replay_prio_push', kw)

    def update(B=B, cap=cap, tree=tree, cur=cur, idx=idx.data_ptr(), pri=pri.data_ptr()):
        return lib.s2d_replay_prio_update(B, cap, tree, cur, idx, pri, st)

    for kw, text in [(dict(B=0), b'batch'), (dict(B=2 ** 24 + 1), b'batch'), (dict(cap=2 ** 30 + 1), b'capacity'), (dict(idx=None), b'non-NULL'),
                     (dict(pri=None), b'non-NULL'), (dict(tree=tree + 4), b'8-byte'), (dict(idx=idx.data_ptr() + 2), b'4-byte'),
                     (dict(idx=tree + 400), b'overlap'), (dict(pri=tree), b'overlap'), (dict(cur=tree + 8), b'overlap')]:
        refused(update(**kw), text, b's2d_replay_prio_update', kw)

    def sample(B=B, tree=tree, cur=cur, ring=rb._ring, **ptrs):
        p = [ptrs.get(k, out[k].data_ptr()) for k in RP.BATCH_FIELDS]
        return lib.s2d_replay_sample_prio(B, D, 1, C.byref(ring), tree, cur, 1, *p, st)

    for kw, text in [(dict(B=0), b'batch'), (dict(B=2 ** 24 + 1), b'batch'), (dict(tree=None), b'non-NULL'), (dict(priority=None), b'non-NULL'),
                     (dict(total=None), b'non-NULL'), (dict(tree=tree + 4), b'8-byte'), (dict(cur=cur + 4), b'8-byte'),
                     (dict(obs=out['obs'].data_ptr() + 8), b'16-byte'), (dict(priority=out['priority'].data_ptr() + 1), b'4-byte'),
                     (dict(priority=tree + 16), b'overlap'), (dict(total=tree), b'overlap'), (dict(index=cur), b'overlap'),
                     (dict(total=out['priority'].data_ptr() + 8), b'overlap'), (dict(next_obs=rb.next_obs.data_ptr()), b'overlap'),
                     (dict(tree=rb.reward.data_ptr()), b'overlap'), (dict(tree=cur - 8), b'overlap')]:
        refused(sample(**kw), text, b's2d_replay_sample_prio', kw)

    same_ring(rb, ring, 'after the refused calls')
    same_tree(rb, start, 'after the refused calls')
    assert all((words_of(out[k]) == 0x7654321).all() for k in RP.BATCH_FIELDS)
    with pytest.raises(ValueError, match='batch'):
        rb.sample(2 ** 24 + 1)
