"""s2d_match_kernel_name() for every instantiation of the cycle kernel an engine can launch: five variants (selected by the
configurations of tests/test_gpu_match_f64.py) times the eight slot states.  bench.py, the profile scripts and the other tests
compare these strings, so they are pinned here as literals.  No launch: the name is a function of the engine's host state."""
import pytest

from test_gpu_match_f64 import KERNELS, _engines

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

STATES = ('none', 'controllers', 'network', 'opponent only', 'two networks', 'policy network', 'two networks, policy', 'see network')
NAMES = {
    'stock rules, own schedule': (
        's2d_match_rollout_kernel<stock rules, own schedule>',
        's2d_match_rollout_kernel<stock rules, own schedule, controllers>',
        's2d_match_rollout_kernel<stock rules, own schedule, network>',
        's2d_match_rollout_kernel<stock rules, own schedule, network>',
        's2d_match_rollout_kernel<stock rules, own schedule, two networks>',
        's2d_match_rollout_kernel<stock rules, own schedule, policy network>',
        's2d_match_rollout_kernel<stock rules, own schedule, two networks, policy>',
        's2d_match_rollout_kernel<stock rules, own schedule, see network>'),
    'stock, stock types': (
        's2d_match_rollout_kernel<stock, stock types>',
        's2d_match_rollout_kernel<stock, stock types, controllers>',
        's2d_match_rollout_kernel<stock, stock types, network>',
        's2d_match_rollout_kernel<stock, stock types, network>',
        's2d_match_rollout_kernel<stock, stock types, two networks>',
        's2d_match_rollout_kernel<stock, stock types, policy network>',
        's2d_match_rollout_kernel<stock, stock types, two networks, policy>',
        's2d_match_rollout_kernel<stock, stock types, see network>'),
    'stock': (
        's2d_match_rollout_kernel<stock>',
        's2d_match_rollout_kernel<stock, controllers>',
        's2d_match_rollout_kernel<stock, network>',
        's2d_match_rollout_kernel<stock, network>',
        's2d_match_rollout_kernel<stock, two networks>',
        's2d_match_rollout_kernel<stock, policy network>',
        's2d_match_rollout_kernel<stock, two networks, policy>',
        's2d_match_rollout_kernel<stock, see network>'),
    'general, illegal defense': (
        's2d_match_rollout_kernel<general, illegal defense>',
        's2d_match_rollout_kernel<general, illegal defense, controllers>',
        's2d_match_rollout_kernel<general, illegal defense, network>',
        's2d_match_rollout_kernel<general, illegal defense, network>',
        's2d_match_rollout_kernel<general, illegal defense, two networks>',
        's2d_match_rollout_kernel<general, illegal defense, policy network>',
        's2d_match_rollout_kernel<general, illegal defense, two networks, policy>',
        's2d_match_rollout_kernel<general, illegal defense, see network>'),
    'general': (
        's2d_match_rollout_kernel<general>',
        's2d_match_rollout_kernel<general, controllers>',
        's2d_match_rollout_kernel<general, network>',
        's2d_match_rollout_kernel<general, network>',
        's2d_match_rollout_kernel<general, two networks>',
        's2d_match_rollout_kernel<general, policy network>',
        's2d_match_rollout_kernel<general, two networks, policy>',
        's2d_match_rollout_kernel<general, see network>'),
}


def test_kernel_names_unchanged():
    from soccer2d_amd.actor import MatchPolicyActor, MatchQNetActor
    assert sorted(NAMES) == sorted(k[0] for k in KERNELS)
    q, q2 = MatchQNetActor(16, 16, 4), MatchQNetActor(16, 16, 4)
    pol, see = MatchPolicyActor(16, 16, 4), MatchQNetActor(16, 16, 4, obs='see')
    for name, kw, _ends in KERNELS:
        eng, _ = _engines(16, **kw)
        steps = (lambda: None,
                 lambda: eng.set_controllers({'left': 'scripted', 'right': 'random'}),
                 lambda: eng.set_network(q, 'left'),
                 lambda: (eng.set_network(None), eng.set_opponent_network(q2, 'right')),
                 lambda: eng.set_network(q, 'left'),
                 lambda: (eng.set_network(None), eng.set_network(pol, 'left')),
                 lambda: eng.set_opponent_network(q2, 'right'),
                 lambda: (eng.enable_vision(), eng.set_network(see, 'left')))
        for state, step, want in zip(STATES, steps, NAMES[name]):
            step()
            assert eng.kernel_name() == want, (name, state)
        eng.close()
