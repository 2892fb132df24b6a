"""The device replay buffer without a GPU: the host restatement (tests/replay_ref.c) is pinned against an independent float64
NumPy loop and against the examples' torch formulation, the known answers of the n-step scan are spelled out, DeviceReplay's
argument checks run on the CPU, and the header, the ctypes mirror and the built library agree on the two entry points."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import replay as RR
from test_capi_exports import HDR, ROOT, declared_functions

NEW = ('s2d_replay_push', 's2d_replay_sample')
GOAL, OUT, TIMEOUT = 1, 2, 3


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return RR.build(tmp_path_factory.mktemp('replay_ref'))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------ independent float64 loop
def numpy_push(rec, first_obs, n_step, gamma, capacity, pos=0):
    """the spec as a plain float64 loop: {slot: (obs_t row, next row, action row, R, discount)}"""
    T, N = rec['reward'].shape
    rew, done, res = rec['reward'].astype(np.float64), rec['done'], rec.get('result')
    act = rec['action'].reshape(T, N, -1)
    out = {}
    for t in range(T):
        for i in range(N):
            R, g, s = rew[t, i], float(gamma), t
            while not done[s, i] and s + 1 < T and s + 1 - t < n_step:
                s += 1
                R += g * rew[s, i]
                g *= gamma
            if done[s, i]:
                nxt, disc = rec['terminal_obs'][s, i], (g if res is not None and res[s, i] == TIMEOUT else 0.0)
            else:
                nxt, disc = rec['obs'][s, i], g
            out[(pos + t * N + i) % capacity] = (first_obs[i] if t == 0 else rec['obs'][t - 1, i], nxt, act[t, i], R, disc)
    return out


@pytest.mark.parametrize('n_step', [1, 2, 3, 11])
@pytest.mark.parametrize('with_result', [True, False])
def test_restatement_equals_float64_loop_where_the_arithmetic_is_exact(L, n_step, with_result):
    """gamma = 0.5 and small integer rewards: every partial sum is a short dyadic rational, exact in fp32 and fp64 alike"""
    rng = np.random.default_rng(5)
    T, N, D, AW, cap, pos = 9, 37, 3, 2, 400, 390
    rec, first = RR.synthetic_record(rng, T, N, D, AW, with_result=with_result)
    rec['reward'] = rng.integers(-3, 4, (T, N)).astype(np.float32)
    ring = RR.Ring(cap, D, AW, fill=0xABABABAB)
    ring.cursor[:] = (pos, 17, 4, 9)
    RR.push(L, ring, rec, first, n_step, 0.5)
    want = numpy_push(rec, first, n_step, 0.5, cap, pos)
    assert len(want) == T * N
    for slot in range(cap):
        if slot not in want:
            assert ring.obs[slot, 0] == 0xABABABAB and bits(ring.reward)[slot] == 0xABABABAB and ring.action[slot, 0] == 0xABABABAB
            continue
        o, nx, a, R, disc = want[slot]
        assert np.array_equal(ring.obs[slot], bits(o)) and np.array_equal(ring.next_obs[slot], bits(nx)), slot
        assert np.array_equal(ring.action[slot], bits(a)), slot
        assert bits(ring.reward)[slot] == bits(np.float32(R)) and bits(ring.discount)[slot] == bits(np.float32(disc)), slot
    assert ring.cursor.tolist() == [(pos + T * N) % cap, min(17 + T * N, cap), 5, 9]


def test_one_step_push_is_the_examples_torch_formulation_word_for_word(L):
    rng = np.random.default_rng(6)
    T, N, D, gamma = 7, 29, 10, 0.99
    rec, first = RR.synthetic_record(rng, T, N, D, 1)
    rec['reward'][0, 0] = -0.0
    rec['reward'][3, 5] = -0.0
    nan = np.array([0x7FC12345, 0xFFC00001], np.uint32).view(np.float32)
    rec['obs'][2, 4, 1], rec['terminal_obs'][2, 4, 7], first[3, 9] = nan[0], nan[1], nan[0]
    rec['done'][2, 4], rec['result'][2, 4] = 1, TIMEOUT
    ring = RR.Ring(T * N, D, 1, fill=0x55555555)
    RR.push(L, ring, rec, first, 1, gamma)
    t_rec = {k: torch.from_numpy(v) for k, v in rec.items()}
    obs_t, act, rew, nxt, disc = RR.torch_formulation(t_rec, torch.from_numpy(first), gamma)
    assert np.array_equal(ring.obs, bits(obs_t.numpy())) and np.array_equal(ring.next_obs, bits(nxt.numpy()))
    assert np.array_equal(ring.action, bits(act.numpy()))
    assert np.array_equal(bits(ring.reward), bits(rew.numpy())) and np.array_equal(bits(ring.discount), bits(disc.numpy()))
    assert bits(ring.reward)[0] == 0x80000000 and ring.obs[0 * N + 3, 9] == 0x7FC12345           # -0.0 and the payload survived
    assert ring.next_obs[2 * N + 4, 7] == 0xFFC00001 and ring.obs[3 * N + 4, 1] == 0x7FC12345


# ------------------------------------------------------------------------------------------ known answers
def one_env(reward, done, result, n_step, gamma, L, with_result=True):
    """one env with D = 1: obs[t] = 10 + t, terminal_obs[t] = 100 + t, first_obs = 9 -> (obs_t, next, R, discount) lists"""
    T = len(reward)
    rec = {'obs': (10 + np.arange(T, dtype=np.float32)).reshape(T, 1, 1), 'terminal_obs': (100 + np.arange(T, dtype=np.float32)).reshape(T, 1, 1),
           'action': np.arange(T, dtype=np.int32).reshape(T, 1), 'reward': np.asarray(reward, np.float32).reshape(T, 1),
           'done': np.asarray(done, np.uint8).reshape(T, 1)}
    if with_result:
        rec['result'] = np.asarray(result, np.uint8).reshape(T, 1)
    ring = RR.Ring(T, 1, 1)
    RR.push(L, ring, rec, np.full((1, 1), 9, np.float32), n_step, gamma)
    assert ring.action[:, 0].tolist() == list(range(T)) and ring.cursor.tolist() == [0, T, 1, 0]
    return (ring.obs.view(np.float32)[:, 0].tolist(), ring.next_obs.view(np.float32)[:, 0].tolist(), ring.reward.tolist(),
            ring.discount.tolist())


def test_known_answers_done_inside_at_the_end_and_twice_in_a_row(L):
    # rewards 1, 2, 4, 8, 16; gamma = 0.5; n_step = 3; dones at t = 1 (Goal), t = 2 (Out: two in a row) and t = 4 = T - 1 (Goal)
    o, nx, R, disc = one_env([1, 2, 4, 8, 16], [0, 1, 1, 0, 1], [0, GOAL, OUT, 0, GOAL], 3, 0.5, L)
    assert o == [9, 10, 11, 12, 13]
    assert nx == [101, 101, 102, 104, 104]          # t=0 stops at the done of t=1; t=3 runs into the done of t=4
    assert R == [1 + 0.5 * 2, 2, 4, 8 + 0.5 * 16, 16]
    assert disc == [0, 0, 0, 0, 0] and all(math.copysign(1, d) == 1 for d in disc)        # +0, not -0


def test_known_answers_timeout_against_goal_and_no_result(L):
    rew, done, res = [1, 2, 4, 8], [0, 1, 0, 1], [0, TIMEOUT, 0, GOAL]
    _, nx, R, disc = one_env(rew, done, res, 2, 0.5, L)
    assert nx == [101, 101, 103, 103] and R == [2, 2, 8, 8]
    assert disc == [0.25, 0.5, 0, 0]                 # the Timeout keeps g (gamma^2 after one extra step, gamma at its own step)
    _, nx2, R2, disc2 = one_env(rew, done, res, 2, 0.5, L, with_result=False)
    assert nx2 == nx and R2 == R and disc2 == [0, 0, 0, 0]                                  # result = NULL: both are terminations


def test_known_answers_horizon_cut_by_the_records_end(L):
    T = 4
    o, nx, R, disc = one_env([1, 2, 4, 8], [0] * T, [0] * T, T + 2, 0.5, L)
    assert o == [9, 10, 11, 12] and nx == [13, 13, 13, 13]                                  # every transition ends at obs[T - 1]
    assert R == [1 + 1 + 1 + 1, 2 + 2 + 2, 4 + 4, 8] and disc == [0.5 ** 4, 0.5 ** 3, 0.5 ** 2, 0.5]


def test_restated_sample_indices_and_fields(L):
    """Philox word b & 3 of counter {b >> 2, samples, stream 11}; multiply-high; the counter advances per call"""
    rng = np.random.default_rng(8)
    cap, D, AW, B, seed = 50, 5, 3, 133, 0x0123456789ABCDEF
    ring = RR.Ring(cap, D, AW)
    for k in ('obs', 'next_obs', 'action'):
        getattr(ring, k)[:] = rng.integers(0, 2 ** 32, getattr(ring, k).shape, dtype=np.uint64).astype(np.uint32)
    ring.reward[:], ring.discount[:] = rng.standard_normal(cap), rng.standard_normal(cap)
    ring.cursor[:] = (7, 31, 2, 0)
    a, b = RR.sample(L, ring, B, seed), RR.sample(L, ring, B, seed)
    assert ring.cursor.tolist() == [7, 31, 2, 2]
    assert not np.array_equal(a['index'], b['index'])
    for n, got in ((0, a), (1, b)):
        idx = np.array([L.replay_index(seed, n, j, 31) for j in range(B)])
        assert np.array_equal(got['index'], idx) and idx.min() >= 0 and idx.max() < 31
        for k in RR.RING_FIELDS:
            assert np.array_equal(bits(got[k]), bits(getattr(ring, k)[idx])), k
    # the four words of one block are four different elements' draws; multiply-high of the extreme words
    assert len({L.replay_index(seed, 0, j, 2 ** 31 - 1) for j in range(4)}) == 4
    ring.cursor[1] = 0
    z = RR.sample(L, ring, 9, seed)
    assert (z['index'] == -1).all() and not z['obs'].any() and not z['next_obs'].any() and not z['action'].any()
    assert not bits(z['reward']).any() and not bits(z['discount']).any()


# ------------------------------------------------------------------------------------------ DeviceReplay argument checks
def cpu_buffer(**kw):
    from soccer2d_amd.replay import DeviceReplay
    return DeviceReplay(**{**dict(capacity=64, obs_dim=4, device='cpu'), **kw})


@pytest.mark.parametrize('kw', [dict(capacity=0), dict(capacity=2 ** 31), dict(obs_dim=0), dict(obs_dim=1025), dict(action_words=9),
                                dict(action_words=0), dict(n_step=0), dict(gamma=float('nan')), dict(gamma=float('inf')),
                                dict(action_dtype=torch.int64), dict(seed=-1)])
def test_constructor_rejects(kw):
    with pytest.raises(ValueError, match='DeviceReplay'):
        cpu_buffer(**kw)


def cpu_record(T=4, N=8, D=4, A=None):
    rec = {'obs': torch.zeros(T, N, D), 'terminal_obs': torch.zeros(T, N, D), 'reward': torch.zeros(T, N),
           'action': torch.zeros((T, N) if A is None else (T, N, A), dtype=torch.int32), 'done': torch.zeros(T, N, dtype=torch.uint8),
           'result': torch.zeros(T, N, dtype=torch.uint8)}
    return rec, torch.zeros(N, D)


def test_push_and_sample_reject_before_any_library_call():
    rb = cpu_buffer()
    assert (rb.size, rb.pos, rb.cursor.tolist()) == (0, 0, [0, 0, 0, 0]) and rb.cursor.dtype == torch.int64
    rec, first = cpu_record()
    big, big_first = cpu_record(T=9, N=8)                                           # 72 > 64
    with pytest.raises(ValueError, match='capacity'):
        rb.push(big, big_first)
    no_term = {k: v for k, v in rec.items() if k != 'terminal_obs'}
    with pytest.raises(ValueError, match='terminal_obs'):
        rb.push(no_term, first)
    for key, bad in (('obs', rec['obs'].double()), ('obs', torch.zeros(4, 8, 5)), ('action', rec['action'].long()),
                     ('action', torch.zeros(4, 8, 2, dtype=torch.int32)), ('done', rec['done'].bool()),
                     ('reward', torch.zeros(4, 8, 1)), ('result', rec['result'].int()), ('terminal_obs', torch.zeros(4, 8, 4)[:, :, ::2])):
        with pytest.raises(ValueError, match=key):
            rb.push({**rec, key: bad}, first)
    with pytest.raises(ValueError, match='first_obs'):
        rb.push(rec, torch.zeros(7, 4))
    with pytest.raises(ValueError, match='batch'):
        rb.sample(0)
    out = rb.alloc_batch(16)
    with pytest.raises(ValueError, match='index'):
        rb.sample(16, out={**out, 'index': out['index'].long()})
    # a well-formed call on a CPU buffer is refused too: there is no CPU path
    with pytest.raises(ValueError, match='GPU'):
        rb.push(rec, first)
    with pytest.raises(ValueError, match='GPU'):
        rb.sample(16)
    rb.clear()
    assert rb.cursor.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ header / mirror / library
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    return _capi.load_library()


def test_replay_entry_points_declared_bound_and_exported(lib):
    from soccer2d_amd import _capi
    names = declared_functions(HDR)
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    for n in NEW:
        assert n in names and n in protos and hasattr(lib, n), n
    assert len(protos['s2d_replay_push'][2]) == 16 and len(protos['s2d_replay_sample'][2]) == 13
    hdr = open(HDR).read()
    assert _capi.S2D_ABI_VERSION == 4 and '#define S2D_ABI_VERSION 4' in hdr and '#define S2D_REPLAY_STREAM 11' in hdr


def test_replay_ring_struct_matches_c(tmp_path):
    from soccer2d_amd import _capi
    prog = tmp_path / 'szr.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                    'sizeof(S2DReplayRing),offsetof(S2DReplayRing,obs),offsetof(S2DReplayRing,next_obs),offsetof(S2DReplayRing,action),'
                    'offsetof(S2DReplayRing,reward),offsetof(S2DReplayRing,discount));return 0;}\n')
    exe = tmp_path / 'szr'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    R = _capi.S2DReplayRing
    assert got == [C.sizeof(R), R.obs.offset, R.next_obs.offset, R.action.offset, R.reward.offset, R.discount.offset]


def test_entry_points_reject_without_a_gpu(lib):
    """argument checks come before any HIP call: every pointer below is a made-up address that is never dereferenced"""
    from soccer2d_amd import _capi
    ring = _capi.S2DReplayRing(100, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000)
    cur, st = 0x60000, None
    rec = (0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000)

    def push(T=4, N=8, D=4, AW=1, n_step=1, gamma=0.99, rec=rec, ring=ring, cur=cur):
        return lib.s2d_replay_push(T, N, D, AW, n_step, gamma, *rec, C.byref(ring) if ring is not None else None, cur, st)

    for kw, text in ((dict(T=0), b'n_steps'), (dict(N=0), b'n_envs'), (dict(D=0), b'obs_dim'), (dict(D=1025), b'obs_dim'),
                     (dict(AW=0), b'action_words'), (dict(AW=9), b'action_words'), (dict(n_step=0), b'n_step'),
                     (dict(gamma=float('nan')), b'finite'), (dict(gamma=float('-inf')), b'finite'), (dict(T=13, N=8), b'capacity'),
                     (dict(N=2 ** 40), b'capacity'), (dict(ring=None), b'ring'),
                     (dict(ring=_capi.S2DReplayRing(0, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000)), b'capacity'),
                     (dict(ring=_capi.S2DReplayRing(2 ** 31, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000)), b'capacity'),
                     (dict(ring=_capi.S2DReplayRing(100, 0x10000, None, 0x30000, 0x40000, 0x50000)), b'non-NULL'),
                     (dict(cur=None), b'non-NULL'), (dict(cur=0x60004), b'8-byte'),
                     (dict(rec=(None,) + rec[1:]), b'non-NULL'), (dict(rec=rec[:5] + (None, None)), b'non-NULL'),
                     (dict(rec=(0x100004,) + rec[1:]), b'16-byte'), (dict(rec=rec[:4] + (0x500002,) + rec[5:]), b'4-byte'),
                     (dict(ring=_capi.S2DReplayRing(100, 0x10008, 0x20000, 0x30000, 0x40000, 0x50000)), b'16-byte'),
                     (dict(ring=_capi.S2DReplayRing(100, 0x10000, 0x20000, 0x30000, 0x40001, 0x50000)), b'4-byte'),
                     (dict(rec=rec[:1] + (0x10000 + 64,) + rec[2:]), b'overlap'),               # obs inside the ring's obs
                     (dict(rec=rec[:5] + (0x60000 + 8, None)), b'overlap'),                      # done inside the cursor
                     (dict(ring=_capi.S2DReplayRing(100, 0x10000, 0x10000 + 160, 0x30000, 0x40000, 0x50000)), b'overlap')):
        assert push(**kw) == _capi.S2D_EINVAL, kw
        assert text in lib.s2d_last_error() and b's2d_replay_push' in lib.s2d_last_error(), (kw, lib.s2d_last_error())
    # D % 4 != 0 needs only 4-byte rows; result may be NULL: both pass the checks, so they are not tried here (they would launch)

    batch = (0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000)

    def sample(B=32, D=4, AW=1, ring=ring, cur=cur, batch=batch):
        return lib.s2d_replay_sample(B, D, AW, C.byref(ring), cur, 1, *batch, st)

    for kw, text in ((dict(B=0), b'batch'), (dict(B=2 ** 31), b'batch'), (dict(D=1025), b'obs_dim'), (dict(AW=9), b'action_words'),
                     (dict(cur=0x60004), b'8-byte'), (dict(batch=batch[:5] + (None,)), b'non-NULL'),
                     (dict(batch=(0x100008,) + batch[1:]), b'16-byte'), (dict(batch=batch[:3] + (0x400002,) + batch[4:]), b'4-byte'),
                     (dict(batch=(0x20000 + 16,) + batch[1:]), b'overlap'), (dict(batch=batch[:5] + (0x60000,)), b'overlap'),
                     (dict(batch=batch[:4] + (0x400000 + 64, 0x600000)), b'overlap')):
        assert sample(**kw) == _capi.S2D_EINVAL, kw
        assert text in lib.s2d_last_error() and b's2d_replay_sample' in lib.s2d_last_error(), (kw, lib.s2d_last_error())
