"""GPU check of the one pack kernel of the streamed-weight MLP (csrc/s2d_wide_pack.hip) through its three users: the workspace
after one call of s2d_debug_wide_forward (input width 10), s2d_gtc_debug_forward (4) and s2d_td_target_q (1, 4, 10, 11, 256) is,
word for word, what a NumPy restatement of the layout gives, and at widths 10 and 4 the three paths leave the same words."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
F = np.float32
N = 65                  # batch rows: more than one wave
GUARD = 64              # words behind the workspace that must stay as they were
# (8,): one tile with padded rows; (12, 20): widths that are no multiples of 16, k-steps 3 then 5; (12, 20, 28): the layer walk
# past two; 1 and 17 outputs: one and two output tiles
CASES = [(h, a) for h in ((8,), (12, 20), (12, 20, 28)) for a in (1, 17)]


def pack(params, n_in, hidden, n_out):
    """the workspace's words: per layer the fragments (jt, s) of 64 words, word l = W[16 jt + (l & 15)][4 s + (l >> 4)] or 0 outside
    the matrix, layer 1 with ceil(n_in / 4) k-steps; behind all fragments every layer's biases, zero-padded to a multiple of 16"""
    frags, biases, off, win = [], [], 0, n_in
    for w in tuple(hidden) + (n_out,):
        ks, m16 = -(-win // 4), -(-w // 16)
        W, b = np.zeros((16 * m16, 4 * ks), F), np.zeros(16 * m16, F)
        W[:w, :win] = params[off:off + w * win].reshape(w, win)
        b[:w] = params[off + w * win:off + w * win + w]
        frags.append(W.reshape(m16, 16, ks, 4).transpose(0, 2, 3, 1).ravel())    # [jt][s][l >> 4][l & 15]
        biases.append(b)
        off, win = off + w * win + w, w
    assert off == params.size
    return np.concatenate(frags + biases)


def distinct_params(rs, n_in, hidden, n_out):
    """every word another value, so that a transposed or shifted word cannot match"""
    count, win = 0, n_in
    for w in tuple(hidden) + (n_out,):
        count, win = count + w * win + w, w
    p = ((rs.permutation(count) + 1) / F(count + 1) - 0.5).astype(F)
    assert np.unique(p).size == count
    return p


def fill(s, hidden, n_out, params, ws, words):
    s.n_hidden, s.n_out, s.activation = len(hidden), n_out, 0
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    s.params, s.workspace, s.workspace_bytes = params.data_ptr(), ws.data_ptr(), words * 4
    return s


def packed_by(path, n_in, hidden, n_out, params):
    """the int32 words of the workspace after one call of `path` ('wide' | 'gtc' | 'td'), guard words checked"""
    from soccer2d_amd import _capi, gtc
    from soccer2d_amd.td import td_workspace_bytes
    lib = gtc.bind(_capi.load_library())
    words = td_workspace_bytes(n_in, hidden, n_out) // 4
    dev = 'cuda:0'
    p = torch.from_numpy(params).to(dev)
    ws = torch.full((words + GUARD,), -3333.0, dtype=torch.float32, device=dev)
    x = torch.rand((N, n_in), dtype=torch.float32, device=dev)
    y = torch.zeros((N, n_out), dtype=torch.float32, device=dev)
    g = torch.zeros((N,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if path == 'td':
        s = fill(_capi.S2DTdNet(), hidden, n_out, p, ws, words)
        s.n_in = n_in
        r, d, t = (torch.zeros((N,), dtype=torch.float32, device=dev) for _ in range(3))
        rc = lib.s2d_td_target_q(N, C.byref(s), None, C.c_void_p(x.data_ptr()), C.c_void_p(r.data_ptr()), C.c_void_p(d.data_ptr()),
                                 C.c_void_p(t.data_ptr()), None, None, None)
        _capi.check(lib, rc, 's2d_td_target_q')
    else:
        assert n_in == {'wide': 10, 'gtc': 4}[path]
        s = fill(_capi.S2DWideNet(), hidden, n_out, p, ws, words)
        s.noise_kind = 0
        fn = 's2d_debug_wide_forward' if path == 'wide' else 's2d_gtc_debug_forward'
        _capi.check(lib, getattr(lib, fn)(C.byref(s), x.data_ptr(), N, y.data_ptr(), g.data_ptr(), None, None), fn)
    torch.cuda.synchronize()
    assert bool((ws[words:] == -3333.0).all()), f'{path}: wrote past the workspace'
    return ws[:words].view(torch.int32)


@pytest.mark.parametrize('hidden,n_out', CASES, ids=[f'{"-".join(map(str, h))}-{a}' for h, a in CASES])
def test_workspace_is_the_packed_network(hidden, n_out):
    from soccer2d_amd.td import td_workspace_bytes
    rs = np.random.RandomState(1000 * sum(hidden) + n_out)
    for n_in in (1, 4, 10, 11, 256):
        params = distinct_params(rs, n_in, hidden, n_out)
        want = pack(params, n_in, hidden, n_out)
        assert want.size == td_workspace_bytes(n_in, hidden, n_out) // 4
        want = torch.from_numpy(want.view(np.int32)).to('cuda:0')
        got = packed_by('td', n_in, hidden, n_out, params)
        assert torch.equal(got, want), f'td n_in={n_in}: {int((got != want).sum())} of {want.numel()} words differ'
        actor = {10: 'wide', 4: 'gtc'}.get(n_in)
        if actor:
            mine = packed_by(actor, n_in, hidden, n_out, params)
            assert torch.equal(mine, want), f'{actor}: {int((mine != want).sum())} of {want.numel()} words differ'
            assert torch.equal(mine, got), f'{actor} and td leave different workspaces'
