"""Host-side checks of the 11v11 see network: the C restatement of the forward pass with the input width as an argument
(tests/see_net_ref.c) against a float64 torch forward and against the 224-input restatement, MatchQNetActor(obs='see')'s packing
and validation, and the S2DMatchSeeNet mirror against the C struct (compiled from include/s2d_match.h)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import match_net as MN
import see_net as SN

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('see_net')
    return SN.build(d), MN.build(d)


def _module(h1, h2, k, seed, dim=192):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(dim, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                               torch.nn.Linear(h2, k))


def _packed(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()


@pytest.mark.parametrize('h1,h2,k', [(16, 16, 1), (32, 48, 5), (64, 64, 16), (48, 32, 64)])
def test_host_forward_against_float64_torch(refs, h1, h2, k):
    L, ML = refs
    m = _module(h1, h2, k, h1 + h2 + k)
    rng = np.random.default_rng(k)
    x = rng.normal(0, 20, (257, 192)).astype(np.float32)
    got = SN.forward(L, x, _packed(m), h1, h2, k)
    want = m.double()(torch.from_numpy(x).double()).detach().numpy()
    assert got.shape == (257, k)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


def test_host_forward_equals_the_224_input_restatement(refs):
    """with the width 224 the forward pass is bitwise tests/match_net_ref.c's: one spec, two widths"""
    L, ML = refs
    m = _module(32, 16, 7, 3, dim=224)
    x = np.random.default_rng(1).normal(0, 5, (64, 224)).astype(np.float32)
    a = SN.forward(L, x, _packed(m), 32, 16, 7, dim=224)
    b = MN.forward(ML, x, _packed(m), 32, 16, 7)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # relu maps NaN and -0 to +0, the argmax never lets a NaN replace the best: a NaN input word gives index 0
    x[0, 5] = np.nan
    assert MN.argmax(ML, SN.forward(L, x[:1], _packed(m), 32, 16, 7, dim=224))[0] == 0


def test_see_actor_packs_in_sequential_order_and_validates():
    from soccer2d_amd.actor import MatchQNetActor
    m = _module(32, 16, 5, 1)
    table = np.arange(25, dtype=np.float32).reshape(5, 5)
    a = MatchQNetActor.from_module(m, table, device='cpu', epsilon=0.2, obs='see')
    assert (a.hidden1, a.hidden2, a.n_actions, a.obs, a.in_dim) == (32, 16, 5, 'see', 192)
    assert a.shapes()[0] == (32, 192)
    assert np.array_equal(a.params.numpy(), _packed(m)) and a.params.numel() == SN.param_count(32, 16, 5)
    assert np.array_equal(a.params.numpy()[:32 * 192].reshape(32, 192), m[0].weight.detach().numpy())   # W1[h1][192] first
    assert np.array_equal(a.table.numpy(), table) and a.table.shape == (5, 5) and a.epsilon == pytest.approx(0.2)
    with torch.no_grad():
        m[0].weight.add_(1.0)
    a.sync()
    assert np.array_equal(a.params.numpy(), _packed(m))
    with pytest.raises(ValueError):
        a.set_table(np.zeros((5, 3)))                    # a [K, 3] table is the agent-row network's
    with pytest.raises(ValueError):
        a.set_table(np.zeros((4, 5)))
    with pytest.raises(ValueError):
        MatchQNetActor.from_module(m, np.zeros((5, 3), dtype=np.float32), device='cpu', obs='see')
    with pytest.raises(ValueError):
        MatchQNetActor.from_module(_module(32, 16, 5, 1, dim=224), table, device='cpu', obs='see')   # wrong input width
    with pytest.raises(ValueError):
        MatchQNetActor.from_module(m, np.zeros((5, 3), dtype=np.float32), device='cpu')            # 192 inputs, agent actor
    with pytest.raises(ValueError):
        MatchQNetActor(device='cpu', obs='state')
    for kw in (dict(hidden1=24), dict(hidden2=80), dict(n_actions=0), dict(n_actions=65)):
        with pytest.raises(ValueError):
            MatchQNetActor(device='cpu', obs='see', **kw)
    with pytest.raises(ValueError):
        a.c_struct(0x7FF)                                # a see actor's struct needs the vision parameters and planes
    # the default actor is unchanged: 224 inputs, a [K, 3] table, an S2DMatchNet
    from soccer2d_amd import _capi_match as M
    d = MatchQNetActor(16, 16, 4, device='cpu')
    assert d.obs == 'agent' and d.shapes()[0] == (16, 224) and d.table.shape == (4, 3)
    assert d.params.numel() == MN.param_count(16, 16, 4) and isinstance(d.c_struct(1), M.S2DMatchNet)
    prm, vis = M.S2DVisionParams(), M.S2DMatchVision(64, 128, 192)
    prm.visible_distance = 3.0
    s = a.c_struct(0x3FF800, prm, vis)
    assert isinstance(s, M.S2DMatchSeeNet)
    assert (s.h1, s.h2, s.n_actions, s.slot_mask) == (32, 16, 5, 0x3FF800)
    assert (s.params, s.epsilon, s.table) == (a.params.data_ptr(), a.epsilon_tensor.data_ptr(), a.table.data_ptr())
    assert s.prm.visible_distance == 3.0 and (s.vis.neck, s.vis.view_width, s.vis.see_wait) == (64, 128, 192)


def test_struct_mirror_matches_the_header(tmp_path):
    from soccer2d_amd import _capi_match as M
    src = tmp_path / 'sz.c'
    fields = ('slot_mask', 'params', 'epsilon', 'table', 'prm', 'vis')
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "s2d_match.h"\nint main(void) { printf("%zu' + ' %zu' * len(fields) +
                   '\\n", sizeof(S2DMatchSeeNet)' + ''.join(f', offsetof(S2DMatchSeeNet, {f})' for f in fields) + '); return 0; }\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = M.S2DMatchSeeNet
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got[0] == 40 + C.sizeof(M.S2DVisionParams) + C.sizeof(M.S2DMatchVision)
    names = {p[0] for p in M.MATCH_PROTOTYPES}
    assert {'s2d_match_set_see_network', 's2d_match_rollout_see'} <= names
