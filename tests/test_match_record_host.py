"""MatchEngine._record, the one check of a rollout record buffer (actions, net_index, agent_obs, logp, see): absent, right and
each way of being wrong, with the messages MatchEngine.rollout raises.  No GPU: a bare engine on the CPU device."""
import pytest

torch = pytest.importorskip('torch')


def _bare_engine(n=3):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine.__new__(MatchEngine)                 # no GPU here: the helper reads the engine's device only
    eng.device, eng.num_envs, eng._h = torch.device('cpu'), n, None
    return eng


CASES = [('actions', (3, 22, 3), torch.float32, "rollout buffer 'actions' must be contiguous float32 [T>=5,3,22,3]"),
         ('net_index', (3, 22), torch.int32, "rollout buffer 'net_index' must be contiguous int32 [T>=5,3,22]"),
         ('agent_obs', (3, 11, 224), torch.float32, "rollout buffer 'agent_obs' must be contiguous float32 [T>=5,3,11,224]"),
         ('logp', (3, 22), torch.float32, "rollout buffer 'logp' must be contiguous float32 [T>=5,3,22]"),
         ('see', (3, 2, 192), torch.float32, "rollout buffer 'see' must be contiguous float32 [T>=5,3,2,192]")]


@pytest.mark.parametrize('name,tail,dtype,message', CASES, ids=[c[0] for c in CASES])
def test_record(name, tail, dtype, message):
    eng, T = _bare_engine(), 5
    out = {}
    t = eng._record(out, name, T, tail, dtype)             # absent: allocated on the engine's device and kept in out
    assert out[name] is t and tuple(t.shape) == (T,) + tail and t.dtype == dtype and t.device == eng.device and t.is_contiguous()
    assert eng._record(out, name, T, tail, dtype) is t     # right: returned as it is
    longer = torch.zeros((T + 2,) + tail, dtype=dtype)
    assert eng._record({name: longer}, name, T, tail, dtype) is longer   # more steps than T are fine
    other = torch.int32 if dtype == torch.float32 else torch.float32
    wrong = {'dtype': torch.zeros((T,) + tail, dtype=other),
             'non-contiguous': torch.zeros((T,) + tail[:-1] + (2 * tail[-1],), dtype=dtype)[..., ::2],
             'short T': torch.zeros((T - 1,) + tail, dtype=dtype),
             'tail': torch.zeros((T,) + tail[:-1] + (tail[-1] + 1,), dtype=dtype),
             'rank': torch.zeros((T,) + tail[:-1], dtype=dtype)}
    assert tuple(wrong['non-contiguous'].shape) == (T,) + tail and not wrong['non-contiguous'].is_contiguous()
    for what, bad in wrong.items():
        with pytest.raises(ValueError) as e:
            eng._record({name: bad}, name, T, tail, dtype)
        assert str(e.value) == message, what
