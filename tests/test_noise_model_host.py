"""CPU-side checks of the selectable movement-noise model (S2DConfig.noise_model, include/s2d.h): the field takes the place of
reserved[0] without moving anything else, make_config maps the names and refuses what makes no sense, and the C validator
agrees.  The HIP library loads without a GPU (as in test_capi_exports.py); nothing here launches a kernel."""
import ctypes as C
import os
import subprocess

import pytest

from soccer2d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _ConfigBefore(C.Structure):
    """S2DConfig as it was before noise_model existed (abi 4): four reserved words behind `noise`."""
    _fields_ = [('abi_version', C.c_uint32), ('struct_bytes', C.c_uint32), ('sp', _capi.S2DServerParams),
                ('task', _capi.S2DReachBallParams), ('seed', C.c_uint64), ('env_id_offset', C.c_int64),
                ('auto_reset', C.c_int32), ('noise', C.c_int32), ('reserved', C.c_int32 * 4)]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    return _capi.load_library()


def test_layout_unchanged():
    assert C.sizeof(_capi.S2DConfig) == C.sizeof(_ConfigBefore)
    assert _capi.S2DConfig.noise_model.offset == _ConfigBefore.reserved.offset
    assert _capi.S2DConfig.reserved.offset == _ConfigBefore.reserved.offset + 4
    for name, *_ in _ConfigBefore._fields_[:-1]:
        assert getattr(_capi.S2DConfig, name).offset == getattr(_ConfigBefore, name).offset, name
    assert _capi.S2D_ABI_VERSION == 4


def test_layout_matches_c_header(tmp_path):
    prog = tmp_path / 'nm.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d.h"\nint main(){printf("%zu %zu %zu %d %d %d\\n",'
                    'sizeof(S2DConfig),offsetof(S2DConfig,noise_model),offsetof(S2DConfig,reserved),'
                    'S2D_NOISE_LATTICE,S2D_NOISE_RCSSSERVER,S2D_ABI_VERSION);return 0;}\n')
    exe = tmp_path / 'nm'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [C.sizeof(_ConfigBefore), _ConfigBefore.reserved.offset, _ConfigBefore.reserved.offset + 4,
                   _capi.NOISE_LATTICE, _capi.NOISE_RCSSSERVER, 4]


def test_default_config_is_lattice(lib):
    cfg = _capi.S2DConfig()
    lib.s2d_default_config(C.byref(cfg))
    assert cfg.noise == 1 and cfg.noise_model == _capi.NOISE_LATTICE and list(cfg.reserved) == [0, 0, 0]


def test_make_config_maps_names(lib):
    from soccer2d_amd.engine import make_config
    assert make_config().noise_model == _capi.NOISE_LATTICE
    assert make_config(noise_model='lattice').noise_model == _capi.NOISE_LATTICE
    assert make_config(noise_model='rcssserver').noise_model == _capi.NOISE_RCSSSERVER
    assert make_config(noise=False, noise_model='lattice').noise_model == _capi.NOISE_LATTICE
    # the default model changes nothing: the bytes equal those of a config that never heard of the field
    assert bytes(memoryview(make_config())) == bytes(memoryview(make_config(noise_model='lattice')))


@pytest.mark.parametrize('bad', ['square', 'RCSSSERVER', '', None, 1, 0, 2])
def test_make_config_rejects_unknown_model(lib, bad):
    from soccer2d_amd.engine import make_config
    with pytest.raises(ValueError, match='noise_model'):
        make_config(noise_model=bad)


def test_make_config_rejects_rcssserver_without_noise(lib):
    from soccer2d_amd.engine import make_config
    with pytest.raises(ValueError, match='noise'):
        make_config(noise=False, noise_model='rcssserver')


def test_c_validator(lib):
    cfg = _capi.S2DConfig()
    lib.s2d_default_config(C.byref(cfg))
    cfg.noise_model = _capi.NOISE_RCSSSERVER
    assert lib.s2d_validate_config(C.byref(cfg)) == _capi.S2D_OK
    for model in (2, -1, 7):
        cfg.noise_model = model
        assert lib.s2d_validate_config(C.byref(cfg)) == _capi.S2D_EINVAL
        assert b'noise_model' in lib.s2d_last_error()
    cfg.noise, cfg.noise_model = 0, _capi.NOISE_RCSSSERVER
    assert lib.s2d_validate_config(C.byref(cfg)) == _capi.S2D_EINVAL
    assert b'noise = 1' in lib.s2d_last_error()
    cfg.noise_model = _capi.NOISE_LATTICE
    assert lib.s2d_validate_config(C.byref(cfg)) == _capi.S2D_OK
    # s2d_create validates before it looks for a device
    cfg.noise_model = 2
    h = C.c_void_p()
    assert lib.s2d_create(C.byref(cfg), 4, 0, None, 0, None, C.byref(h)) == _capi.S2D_EINVAL and not h.value

