"""The (return code, s2d_last_error() text) of every refusal the fused-actor tests provoke, against tests/golden/actor_refusals.json.

The file was recorded from the library and Python of the commit before the entry points were put on one host path, so a text
that moves or changes with the shared helpers shows.  To record it again, run the GPU tests that call refused() --
test_gpu_actor_refusals.py and the rejection tests of test_gpu_{qnet,ddpg,mlp,wide,ppo}_actor.py -- with
S2D_ACTOR_REFUSALS_WRITE=<path of a new json file> in the environment: they then write what they see, merged into that file,
instead of comparing.  The texts hold no addresses."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'actor_refusals.json')
_write = os.environ.get('S2D_ACTOR_REFUSALS_WRITE')
_golden = None


def refused(lib, key, rc):
    """the call that has just returned `rc` was refused as the golden file has it under `key`; returns the text"""
    global _golden
    from soccer2d_amd import _capi
    text = lib.s2d_last_error().decode()
    assert rc == _capi.S2D_EINVAL, (key, rc, text)
    if _write:
        seen = {}
        if os.path.exists(_write):
            with open(_write) as f:
                seen = json.load(f)
        assert seen.get(key, [rc, text]) == [rc, text], f'{key} names two refusals: {seen[key]} and {[rc, text]}'
        seen[key] = [rc, text]
        with open(_write, 'w') as f:
            json.dump(seen, f, indent=0, sort_keys=True)
        return text
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)
    assert key in _golden, f'{key} is not in {GOLDEN}'
    assert [rc, text] == _golden[key], (key, [rc, text], _golden[key])
    return text
