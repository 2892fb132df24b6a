"""CPU checks of the one host path of the actor-critic TD targets (csrc/s2d_td.hip, td_target_actor_critic): s2d_td_target_ac,
s2d_td_target_td3, s2d_td_target_sac and s2d_debug_td_target_sac refuse the same bad call with the same text behind their own
prefix, before any HIP call (every array here is host memory or NULL: a refused call touches no device).  The texts are pinned
as literals: they are what the library said when each entry point had a copy of the checks.  The one place where the texts
differ is the critic-shape refusal, which names the head's rule for the critics' input width."""
import ctypes as C

import pytest

ENTRIES = ('s2d_td_target_ac', 's2d_td_target_td3', 's2d_td_target_sac', 's2d_debug_td_target_sac')
SAC = ENTRIES[2:]
NULL_CRITIC = 'actor and critic1 must be non-NULL'
WRONG_WIDTH = {False: "critic1 is 13-12-20-1, the actor 10-12-20-2: a critic's n_in must be the actor's n_in + n_out, its n_out 1",
               True: "critic1 is 13-12-20-1, the actor 10-12-20-4: a critic's n_in must be the actor's n_in + n_out / 2, its n_out 1"}
WRONG_OUT = {False: "critic2 is 12-12-20-2, the actor 10-12-20-2: a critic's n_in must be the actor's n_in + n_out, its n_out 1",
             True: "critic2 is 12-12-20-2, the actor 10-12-20-4: a critic's n_in must be the actor's n_in + n_out / 2, its n_out 1"}
SHARED = 'two networks share a workspace: every network of a call needs its own'
MISALIGNED = 'the optional outputs must be 4-byte aligned device pointers (or NULL)'


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    return _capi.load_library()


class Nets:
    """an actor with two action words and two critics, on host arrays that are aligned as the ABI asks (never read)"""

    def __init__(self, lib, sac, critic_in=12, critic2_out=1):
        self.keep = []
        self.actor = self.net(lib, 10, 4 if sac else 2)
        self.critic1 = self.net(lib, critic_in, 1)
        self.critic2 = self.net(lib, 12, critic2_out)
        self.words = (C.c_double * 64)()                                     # 8-byte aligned: batch arrays, alpha, noise, draws

    def net(self, lib, n_in, n_out):
        from soccer2d_amd import _capi
        s = _capi.S2DTdNet()
        s.n_in, s.n_hidden, s.activation, s.n_out = n_in, 2, 1, n_out
        s.hidden[0], s.hidden[1] = 12, 20
        s.workspace_bytes = lib.s2d_td_workspace_bytes(C.byref(s))
        params, ws = (C.c_float * 4096)(), (C.c_char * (s.workspace_bytes + 256))()
        self.keep += [params, ws]
        s.params = C.addressof(params) + (-C.addressof(params)) % 16
        s.workspace = C.addressof(ws) + (-C.addressof(ws)) % 256
        return s


def call(lib, entry, nets, critic1=True, out_q=0, out_logp=0, draws=72):
    """the entry point on a batch of one with good batch arrays; out_q / out_logp: byte offsets that misalign them (0: NULL);
    draws: the byte where the counter word stands"""
    w = C.addressof(nets.words)
    a = [1, C.byref(nets.actor), C.byref(nets.critic1) if critic1 else None, C.byref(nets.critic2), w, w + 8, w + 16]
    outs = [w + 24, (w + 32 + out_q) if out_q else None, None]
    if entry == 's2d_td_target_ac':
        a += outs
    elif entry == 's2d_td_target_td3':
        a += [w + 64, w + draws, 7] + outs                                    # noise, draws, seed
    else:
        a += [w + 64, w + draws, 7] + ([1] if entry == 's2d_debug_td_target_sac' else []) + outs   # alpha, draws, seed
        a += [(w + 40 + out_logp) if out_logp else None]
    rc = getattr(lib, entry)(*a, None)
    assert rc != 0
    return lib.s2d_last_error().decode()


@pytest.mark.parametrize('entry', ENTRIES)
def test_four_entry_points_refuse_alike(lib, entry):
    sac = entry in SAC
    assert call(lib, entry, Nets(lib, sac), critic1=False) == f'{entry}: {NULL_CRITIC}'
    assert call(lib, entry, Nets(lib, sac, critic_in=13)) == f'{entry}: {WRONG_WIDTH[sac]}'
    assert call(lib, entry, Nets(lib, sac, critic2_out=2)) == f'{entry}: {WRONG_OUT[sac]}'
    for a, b in (('actor', 'critic1'), ('actor', 'critic2'), ('critic1', 'critic2')):
        nets = Nets(lib, sac)
        getattr(nets, b).workspace = getattr(nets, a).workspace + 256         # inside the other's (both hold more than 256 bytes)
        assert call(lib, entry, nets) == f'{entry}: {SHARED}'
    assert call(lib, entry, Nets(lib, sac), out_q=2) == f'{entry}: {MISALIGNED}'
    if sac:
        assert call(lib, entry, Nets(lib, sac), out_logp=1) == f'{entry}: {MISALIGNED}'


def test_a_good_call_gets_past_the_shared_checks(lib):
    """the refusals above are the shared path's: a good call reaches the head's own words, each entry point's own text"""
    for entry in ENTRIES[1:]:
        assert call(lib, entry, Nets(lib, entry in SAC), draws=76) == f'{entry}: draws must be a non-NULL, 8-byte aligned device pointer'
