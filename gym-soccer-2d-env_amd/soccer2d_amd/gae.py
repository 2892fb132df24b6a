"""gae(): generalised advantage estimation over a time-major record in one launch (s2d_gae in include/s2d.h): the backward scan
of SB3's ``RolloutBuffer.compute_returns_and_advantage`` with its time-limit bootstrap, one lane per env, instead of a T-step
Python loop of small elementwise launches.  Engine-independent: any [T, N] record (reach-ball, 11v11 with agents flattened into
N) on one device."""
import ctypes as C
import math

import torch

from . import _capi


def _arr(name, t, dtype, shape, device):
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != device or not t.is_contiguous():
        raise ValueError(f'gae: {name} must be a contiguous {dtype} tensor of shape {shape} on {device}')
    return C.c_void_p(t.data_ptr())


def gae(reward, done, value, last_value, gamma, lam, result=None, terminal_value=None, out=None):
    """advantage, return = GAE(gamma, lam) of a record: reward float32 [T,N], done uint8 [T,N], value float32 [T,N] (V of the
    observation action t was chosen from), last_value float32 [N] (V of the observation after the last step).  With result
    uint8 [T,N] and terminal_value float32 [T,N] (V of the terminal observations; only the Timeout entries are read), a
    Timeout's reward is bootstrapped with gamma * terminal_value, as SB3 does.  out = (advantage, ret) float32 [T,N] to write
    into (not the inputs); returns them.  Stream-ordered on torch's current stream, capturable."""
    if not torch.is_tensor(reward) or reward.dim() != 2 or reward.device.type != 'cuda':
        raise ValueError('gae: reward must be a [T, N] tensor on a GPU')
    T, N = reward.shape
    if T < 1 or N < 1:
        raise ValueError('gae: T and N must be >= 1')
    if not (math.isfinite(gamma) and math.isfinite(lam)):
        raise ValueError('gae: gamma and lam must be finite')
    if (result is None) != (terminal_value is None):
        raise ValueError('gae: result and terminal_value go together (both or neither)')
    dev, f32, shape = reward.device, torch.float32, (T, N)
    ptrs = [_arr('reward', reward, f32, shape, dev), _arr('done', done, torch.uint8, shape, dev), _arr('value', value, f32, shape, dev),
            _arr('last_value', last_value, f32, (N,), dev),
            None if result is None else _arr('result', result, torch.uint8, shape, dev),
            None if terminal_value is None else _arr('terminal_value', terminal_value, f32, shape, dev)]
    if out is None:
        out = (torch.empty(shape, dtype=f32, device=dev), torch.empty(shape, dtype=f32, device=dev))
    adv, ret = out
    pa, pr = _arr('out[0]', adv, f32, shape, dev), _arr('out[1]', ret, f32, shape, dev)
    lib = _capi.load_library()
    with torch.cuda.device(dev):
        rc = lib.s2d_gae(T, N, *ptrs, float(gamma), float(lam), pa, pr, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _capi.check(lib, rc, 's2d_gae')
    return adv, ret
