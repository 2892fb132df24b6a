"""What the GPU tests of the scripted team share (tests/test_gpu_match_scripted_*.py): written states into the engine's planes, one
cycle with a controller table, the record before the engine's gating.  TEST INFRASTRUCTURE."""
import numpy as np

import match_oracle as MO
import scripted_f64 as F

DEV = 'cuda:0'
FIELDS = MO.STATE_FIELDS
ALL_SCRIPTED = [2] * 22


def engine(cfg, n, table=ALL_SCRIPTED):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine(n, DEV, cfg=cfg)
    eng.set_controllers(table)
    eng.reset()
    return eng


def load(eng, state, keys=FIELDS):
    """write a state into the engine's planes (the way test_gpu_match_symmetry._load does); keys: the words to write"""
    import torch
    for k in keys:
        getattr(eng, k).copy_(torch.as_tensor(np.ascontiguousarray(state[k]), device=DEV))


def load_scene(eng, state):
    """a scene names the words the controller reads; every other word stays the kick-off's, the velocities are zero"""
    eng.reset()
    load(eng, state, F.KEYS + ('vx', 'vy'))


def read(eng, keys=F.KEYS):
    return {k: getattr(eng, k).cpu().numpy() for k in keys}


def cycle(eng, T=1, **kw):
    """T cycles in one launch -> the action record [T, n, 22, 3] (numpy) and the launch's other records"""
    out = eng.rollout(T, with_obs=False, record_actions=True, **kw)
    return out['actions'].cpu().numpy(), out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same_words(got, want, tag):
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        i = tuple(bad[0][:-1])
        raise AssertionError(f'{tag}: {len(bad)} words differ; first at {tuple(bad[0])}: device {got[i]} host {want[i]}')
