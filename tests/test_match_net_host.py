"""Host-side checks of the 11v11 network slots: the C restatement (tests/match_net_ref.c) against a float64 torch forward, its
argmax and threshold, the numpy exploration draws, MatchQNetActor's packing and validation, and the S2DMatchNet mirror against
the C struct (compiled from include/s2d_match.h)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import match_net as MN
import qnet_ref as Q

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return MN.build(tmp_path_factory.mktemp('match_net'))


def _module(h1, h2, k, seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(224, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                               torch.nn.Linear(h2, k))


def _packed(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()


@pytest.mark.parametrize('h1,h2,k', [(16, 16, 1), (32, 48, 5), (64, 64, 16), (48, 32, 64)])
def test_host_forward_against_float64_torch(ref, h1, h2, k):
    m = _module(h1, h2, k, h1 + h2 + k)
    rng = np.random.default_rng(k)
    x = rng.normal(0, 20, (257, 224)).astype(np.float32)
    got = MN.forward(ref, x, _packed(m), h1, h2, k)
    want = m.double()(torch.from_numpy(x).double()).detach().numpy()
    assert got.shape == (257, k)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


def test_argmax_threshold_and_draws(ref):
    q = np.array([[1, 3, 3, 0], [np.nan, 1, 2, 2], [0, np.nan, -1, 5], [-0.0, 0.0, -1, -2]], dtype=np.float32)
    assert MN.argmax(ref, q).tolist() == [1, 0, 3, 0]
    assert MN.threshold(ref, 1.0) == 2 ** 32 and MN.threshold(ref, 0.0) == 0 and MN.threshold(ref, float('nan')) == 0
    assert MN.threshold(ref, 0.25) == 2 ** 30 and MN.threshold(ref, -1.0) == 0
    # the draw of (match gid, slot) at tick t is Philox block (gid, t, stream 7 << 16 | slot) under the seed
    wx, wy = MN.draws(0x5EED, np.array([3, 2 ** 33 + 1]), np.array([5, -1]), [0, 21])
    for i, (gid, tick) in enumerate(((3, 5), (2 ** 33 + 1, 2 ** 32 - 1))):
        for j, slot in enumerate((0, 21)):
            w = Q.philox(gid & 0xFFFFFFFF, gid >> 32, tick, (7 << 16) | slot, 0x5EED, 0)
            assert (int(wx[i, j]), int(wy[i, j])) == (int(w[0]), int(w[1]))


def test_actor_packs_in_sequential_order_and_validates():
    from soccer2d_amd.actor import MatchQNetActor
    m = _module(32, 16, 5, 1)
    table = np.arange(15, dtype=np.float32).reshape(5, 3)
    a = MatchQNetActor.from_module(m, table, device='cpu', epsilon=0.2)
    assert (a.hidden1, a.hidden2, a.n_actions) == (32, 16, 5)
    assert np.array_equal(a.params.numpy(), _packed(m)) and a.params.numel() == MN.param_count(32, 16, 5)
    assert np.array_equal(a.table.numpy(), table) and a.epsilon == pytest.approx(0.2)
    with torch.no_grad():
        m[0].weight.add_(1.0)
    a.sync()
    assert np.array_equal(a.params.numpy(), _packed(m))
    a.epsilon = 0.0
    assert float(a.epsilon_tensor) == 0.0
    s = a.c_struct(0x7FF)
    assert (s.h1, s.h2, s.n_actions, s.slot_mask) == (32, 16, 5, 0x7FF) and s.table == a.table.data_ptr()
    for kw in (dict(hidden1=24), dict(hidden2=80), dict(hidden1=128), dict(n_actions=0), dict(n_actions=65)):
        with pytest.raises(ValueError):
            MatchQNetActor(device='cpu', **kw)
    with pytest.raises(ValueError):
        a.set_table(np.zeros((4, 3)))
    bad = torch.nn.Sequential(torch.nn.Linear(10, 32), torch.nn.ReLU(), torch.nn.Linear(32, 16), torch.nn.ReLU(),
                              torch.nn.Linear(16, 5))
    with pytest.raises(ValueError):
        MatchQNetActor.from_module(bad, table, device='cpu')
    bad = torch.nn.Sequential(torch.nn.Linear(224, 32), torch.nn.Tanh(), torch.nn.Linear(32, 16), torch.nn.ReLU(),
                              torch.nn.Linear(16, 5))
    with pytest.raises(ValueError):
        MatchQNetActor.from_module(bad, table, device='cpu')
    with pytest.raises(ValueError):
        MatchQNetActor.from_module(_module(24, 16, 5, 2), table, device='cpu')


def test_struct_mirror_matches_the_header(tmp_path):
    from soccer2d_amd import _capi_match as M
    src = tmp_path / 'sz.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "s2d_match.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(S2DMatchNet), offsetof(S2DMatchNet, slot_mask), offsetof(S2DMatchNet, params), '
                   'offsetof(S2DMatchNet, epsilon), offsetof(S2DMatchNet, table)); return 0; }\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = M.S2DMatchNet
    assert got == [C.sizeof(S), S.slot_mask.offset, S.params.offset, S.epsilon.offset, S.table.offset] == [40, 12, 16, 24, 32]
    assert M.MATCH_ST_NET == 7 and M.MATCH_NET_WIDTHS == (16, 32, 48, 64)
    names = {p[0] for p in M.MATCH_PROTOTYPES}
    assert {'s2d_match_set_network', 's2d_match_rollout_net'} <= names
