"""The on-policy entry points (s2d_rollout_policy, s2d_gae, s2d_debug_policy_head) are declared in include/s2d.h, bound by the
ctypes mirror and exported by the built library; S2DPolicyNet has the C struct's size and the ABI version is unchanged."""
import ctypes as C
import os
import subprocess

import pytest

from test_capi_exports import HDR, ROOT, declared_functions

NEW = ('s2d_rollout_policy', 's2d_gae', 's2d_debug_policy_head')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    return _capi.load_library()


def test_policy_entry_points_declared_bound_and_exported(lib):
    from soccer2d_amd import _capi
    names = declared_functions(HDR)
    bound = {p[0] for p in _capi.PROTOTYPES}
    for n in NEW:
        assert n in names and n in bound and hasattr(lib, n), n
    assert _capi.S2D_ABI_VERSION == 4 and '#define S2D_ABI_VERSION 4' in open(HDR).read()


def test_policy_struct_size_matches_c(tmp_path):
    from soccer2d_amd import _capi
    prog = tmp_path / 'szp.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                    'sizeof(S2DPolicyNet),offsetof(S2DPolicyNet,params),offsetof(S2DPolicyNet,log_std),'
                    'offsetof(S2DPolicyNet,deterministic));return 0;}\n')
    exe = tmp_path / 'szp'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    P = _capi.S2DPolicyNet
    assert got == [C.sizeof(P), P.params.offset, P.log_std.offset, P.deterministic.offset]


def test_gae_and_head_reject_without_a_gpu(lib):
    """argument checks come before any HIP call"""
    from soccer2d_amd import _capi
    assert lib.s2d_gae(0, 4, None, None, None, None, None, None, 0.99, 0.95, None, None, None) == _capi.S2D_EINVAL
    assert b'n_steps' in lib.s2d_last_error()
    assert lib.s2d_gae(4, 4, 16, 16, 16, 16, None, None, float('nan'), 0.95, 16, 16, None) == _capi.S2D_EINVAL
    assert b'finite' in lib.s2d_last_error()
    assert lib.s2d_gae(4, 4, 16, 16, 16, 16, 16, None, 0.99, 0.95, 16, 16, None) == _capi.S2D_EINVAL
    assert b'go together' in lib.s2d_last_error()
    assert lib.s2d_debug_policy_head(0, 65, 16, None, 16, 16, 1, 0, 4, 16, 16, None) == _capi.S2D_EINVAL
    assert lib.s2d_debug_policy_head(2, 1, 16, 16, 16, 16, 1, 0, 4, 16, 16, None) == _capi.S2D_EINVAL
