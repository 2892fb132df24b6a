"""Cost of the vision layer at 8 192 matches: s2d_match_see (full mask) and s2d_match_vision_step, and in the same process on the
same device s2d_match_agent_obs (full mask) -- the ratio within one run is the number to quote, absolutes differ between devices
and days.  Each call is captured K times into one graph; the first replays are dropped; the median of R timed replays (device
events), the arms alternating.  Bytes are the algorithmic ones: N * 22 * 768 (see), N * 22 * 896 (agent_obs), and for
vision_step the three planes read and written plus the card plane and the actions read.

The vision planes are held fixed while see is timed: they are snapshotted once in a state where EVERY active agent is fresh (one
vision_step after a reset: the full path of the kernel -- cone, grid, changes, draws, ranks) and copied back, outside the timed
region, before every replay; vision_step's own replays (and its warm-up calls) are what would otherwise move them.  A second see
arm runs on the same planes with see_wait one lower, where nobody is fresh and the kernel writes self and game words only: the
cheapest path, the other end of the range.  After the timed replays the fresh and seen shares are read back from the rows the
last replays wrote, and the script fails if they are not those of the snapshot.

  python profiles/experiments/match_see_cost.py [out.txt]      (default: profiles/r06/match_see_cost.txt; lines from NOTES on,
                                                                 added by hand, are kept when the file is rewritten)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gym-soccer-2d-env_amd')]
import torch  # noqa: E402
from soccer2d_amd._capi_match import SEE_FIELDS as F  # noqa: E402
from soccer2d_amd.match import MatchEngine  # noqa: E402

N, K, DROP, R = 8192, 50, 5, 15
ROOF = 8.0e12                                              # HBM3E peak of the MI355X, bytes / s
CARD_RED = 2
OUT = os.path.join(ROOT, 'profiles', 'r06', 'match_see_cost.txt')
NOTES = '# ---- notes added by hand (not produced by the script; kept when it rewrites the file) ----'


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(K):
            fn()
    return g


def shares(rows):
    """(fresh share of the active agents, seen share of the player rows, ball-seen share) of see rows [N, 22, 192]"""
    active = rows[..., F['self.card']] < CARD_RED
    fresh = rows[..., F['self.fresh']][active]
    return (float(fresh.double().mean()), float((rows[..., F['players.level']] > 0).double().mean()),
            float((rows[..., F['ball.level']] > 0).double().mean()))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else OUT
    eng = MatchEngine(N, 'cuda:0', noise=True)
    eng.enable_vision()
    eng.reset()
    eng.rollout(40, with_obs=False)
    view = torch.zeros((N, 22, 2), dtype=torch.float32, device='cuda:0')
    view[..., 0] = 10.0
    eng.vision_step(view)                                  # the first step after a reset: every active agent is fresh
    planes = (eng.neck, eng.view_width, eng.see_wait)
    fresh_state = tuple(t.clone() for t in planes)
    stale_state = (fresh_state[0], fresh_state[1], fresh_state[2] - 1)   # one cycle later on the timer: nobody is fresh

    def put(state):
        for t, s in zip(planes, state):
            t.copy_(s)

    see = torch.empty((N, 22, 192), dtype=torch.float32, device='cuda:0')
    see_stale = torch.empty_like(see)
    obs = torch.empty((N, 22, 224), dtype=torch.float32, device='cuda:0')
    before = shares(eng.see('all', out=see))
    assert before[0] == 1.0, before
    # name, the call, the planes it starts from, bytes
    arms = [('see(all), all fresh', lambda: eng.see('all', out=see), fresh_state, N * 22 * 768),
            ('see(all), nobody fresh', lambda: eng.see('all', out=see_stale), stale_state, N * 22 * 768),
            ('agent_observations(all)', lambda: eng.agent_observations('all', out=obs), fresh_state, N * 22 * 896),
            ('vision_step', lambda: eng.vision_step(view), fresh_state, N * 24 * 4 * 7 + N * 22 * 8)]
    graphs = []
    for name, fn, state, _ in arms:
        put(state)
        graphs.append(graph_of(fn))
    times = {name: [] for name, _, _, _ in arms}
    for rep in range(DROP + R):
        for (name, _, state, _), g in zip(arms, graphs):
            put(state)                                     # not timed: the events below are recorded after these copies
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            if rep >= DROP:
                times[name].append(a.elapsed_time(b) * 1e-3 / K)
    # what the timed replays really saw: the rows their last calls wrote
    after, after_stale = shares(see), shares(see_stale)
    assert after == before, (before, after)
    assert after_stale == (0.0, 0.0, 0.0), after_stale
    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    ao = med['agent_observations(all)']
    lines = ['# vision layer (s2d_match_see, s2d_match_vision_step): cost at 8 192 matches on one device, beside s2d_match_agent_obs in '
             'the same process',
             '# profiles/experiments/match_see_cost.py (device events around graph replays; bytes = the algorithmic ones)',
             f'# {torch.cuda.get_device_name(0)}; {N} matches; graphs of {K} calls, {DROP} replays dropped, median of {R}, arms alternating',
             '# state: 40 played cycles (noise on), then one vision_step (neck +10); the vision planes are restored before every replay',
             f'# rows written by the last timed replays, all fresh: fresh {after[0]:.3f} of the active agents, '
             f'{after[1]:.3f} of the player rows seen, ball seen by {after[2]:.3f}',
             f'# rows written by the last timed replays, nobody fresh: fresh {after_stale[0]:.3f}, seen {after_stale[1]:.3f}']
    for name, _, _, nbytes in arms:
        v = times[name]
        lines.append(f'{name:26s} {med[name] * 1e6:8.2f} us/call  {nbytes / 1e6:7.1f} MB  {nbytes / med[name] / 1e12:5.2f} TB/s  '
                     f'{nbytes / med[name] / ROOF:5.3f} of the 8 TB/s roofline  min {min(v) * 1e6:.2f} max {max(v) * 1e6:.2f}')
    for name in ('see(all), all fresh', 'see(all), nobody fresh'):
        lines.append(f"{name} / agent_observations(all) = {med[name] / ao:.3f}; with vision_step = {(med[name] + med['vision_step']) / ao:.3f}")
    print('\n'.join(lines), flush=True)
    kept = []
    if os.path.exists(out_path):
        old = open(out_path).read().split('\n')
        if NOTES in old:
            kept = old[old.index(NOTES):]
    open(out_path, 'w').write('\n'.join(lines + kept).rstrip('\n') + '\n')
    eng.close()


if __name__ == '__main__':
    main()
