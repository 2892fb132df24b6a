"""The audio layer (MatchEngine.hear_step: s2d_match_hear_step) at 8 192 matches, with 2, 11 and 22 speakers per match, beside the
s2d_match_see call of the same engine and beside a torch formulation of the same rows, in ONE process, on the state of a played
match (scripted against scripted, noise on).

  see            MatchEngine.see('all'): the 180 224 see rows of the current state.
  hear_K         one hear_step with K speakers per match (K = 2: one per team; 11: half of each team; 22: everybody), every
                 capacity full, a quarter of the listeners attending a teammate.
  torch_K        the same rows from torch ops: own-frame pairwise distances [N, 22, 22], the candidate masks, a masked argmin over
                 random keys per side (torch's generator in the place of the Philox block, so the winners differ; the work is the
                 same), a gather of the payloads, the direction by atan2, the quantisation, the row assembled by cat.  The
                 capacities and attention are updated as well.

Protocol (that of belief_rate.py): every arm is warmed up for `--warmup` seconds of back-to-back work, then `--regions` timed
regions per arm, the arms alternating; a region is a number of calls (sized to about `--region-seconds`) between two host clocks
that end in a device synchronise.  Reported per arm: the median region, the lowest and the highest, in microseconds per call; for
the hear arms the bytes the step must move -- per match 4 planes of 96 B in (x, y, body, card), the neck plane, three hear planes
in and out, 22 say rows of 48 B in, 22 hear rows of 128 B out, tick and done -- over the median time, as a fraction of an 8 TB/s
roofline (at 8 192 matches that is 40 MB, which fits the Infinity Cache: the fraction says how far the call is from the least
time HBM would allow, not that HBM is what it reads from).  No threshold: the numbers are reported.

Prints one JSON object; profiles/r24/hear_rate.json holds a run.
    python profiles/experiments/hear_rate.py [--regions 5] [out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'gym-soccer-2d-env_amd'))

import torch  # noqa: E402

from soccer2d_amd.match import MatchEngine  # noqa: E402

ROOFLINE = 8.0e12
# per match: x, y, body, card, neck in; cap_our, cap_opp, attention in and out; say in; hear out; tick, done
MATCH_BYTES = 5 * 96 + 3 * 2 * 96 + 22 * 48 + 22 * 128 + 4 + 1


def region(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count


def warm(fn, seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def torch_hear(eng, say, prm):
    """the hear rows of the current state in torch ops (the draw from torch's generator); returns [N, 22, 32]"""
    N, dev = eng.num_envs, eng.device
    sg = torch.cat([torch.ones(11, device=dev), -torch.ones(11, device=dev)])
    right = torch.arange(22, device=dev) >= 11
    body = torch.where(right, torch.where(eng.body[:, :22] > 0, eng.body[:, :22] - 180, eng.body[:, :22] + 180), eng.body[:, :22])
    face = body + eng.neck[:, :22]
    # dx[e, p, j] = sg_p * (x_j - x_p) on raw values = own-frame difference
    dx = (eng.x[:, None, :22] - eng.x[:, :22, None]) * sg[None, :, None]
    dy = (eng.y[:, None, :22] - eng.y[:, :22, None]) * sg[None, :, None]
    d = torch.sqrt(dx * dx + dy * dy)
    alive = eng.card[:, :22] < 2
    said = (say[..., 0] != 0) & ~torch.isnan(say[..., 0]) & alive
    eye = torch.eye(22, dtype=torch.bool, device=dev)
    cand = said[:, None, :] & (d <= prm['cut']) & ~eye[None] & alive[:, :, None]
    same = right[:, None] == right[None, :]
    pay = torch.round(torch.nan_to_num(say[..., 2:]).clamp(-1, 1) * prm['half']) * (1.0 / prm['half'])
    att = eng.attention[:, :22]
    att_raw = torch.where(att < 0, att, torch.where(right[None, :], (att + 11) % 22, att))
    keys = torch.rand((N, 22, 22), device=dev)
    keys = torch.where(torch.arange(22, device=dev)[None, None, :] == att_raw[:, :, None], -1.0, keys)   # the attended one first
    recs = []
    for side, cap in ((same, eng.cap_our), (~same, eng.cap_opp)):
        c = cand & side[None]
        count = c.sum(dim=2)
        cp = torch.clamp(cap[:, :22] + prm['inc'], max=prm['max'])
        win = torch.where(c, keys, 2.0).argmin(dim=2)
        heard = (count > 0) & (cp >= prm['decay'])
        cp = cp - prm['decay'] * heard
        cap[:, :22] = cp
        wdx, wdy = dx.gather(2, win[..., None])[..., 0], dy.gather(2, win[..., None])[..., 0]
        ang = torch.rad2deg(torch.atan2(wdy, wdx)) - face
        ang = torch.round(torch.remainder(ang + 180.0, 360.0) - 180.0)
        h = heard.float()
        sender = (win % 11 + 1).float() * h if side is same else torch.zeros_like(h)
        head = torch.stack([h, sender, ang * h, (count - heard.long()).float(), cp.float(),
                            (att + 1).float() if side is same else torch.zeros_like(h)], dim=2)
        recs += [head, pay.gather(1, win[..., None].expand(N, 22, 10)) * h[..., None]]
    return torch.cat(recs, dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--matches', type=int, default=8192)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--region-seconds', type=float, default=0.3)
    ap.add_argument('--warmup', type=float, default=0.5)
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hear_rate.py measures on the GPU: no device found')
    dev, N = 'cuda:0', a.matches
    eng = MatchEngine(N, dev, noise=True, seed=24)
    eng.set_controllers({'left': 'scripted', 'right': 'scripted'})
    eng.enable_vision()
    eng.enable_hearing(hear_max=1000, hear_inc=1000)          # full capacities in every call: every call delivers
    eng.reset()
    eng.rollout(64, with_obs=False)
    eng.vision_step()
    g = torch.Generator(device=dev).manual_seed(24)
    says = {}
    for k, slots in ((2, [5, 16]), (11, [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20]), (22, list(range(22)))):
        s = torch.zeros((N, 22, 12), device=dev)
        s[:, slots, 0] = 1.0
        s[..., 1] = torch.randint(1, 12, (N, 22), device=dev, generator=g).float() * (torch.rand((N, 22), device=dev, generator=g) < 0.25)
        s[..., 2:] = torch.rand((N, 22, 10), device=dev, generator=g) * 2 - 1
        says[k] = s
    rows = torch.empty((N, 22, 192), dtype=torch.float32, device=dev)
    prm = {'cut': 50.0, 'half': 36.0, 'inc': 1000, 'max': 1000, 'decay': 1}
    arms = [('see', lambda: eng.see('all', out=rows))]
    for k in (2, 11, 22):
        arms.append((f'hear_{k}', lambda k=k: eng.hear_step(says[k])))
        arms.append((f'torch_{k}', lambda k=k: torch_hear(eng, says[k], prm)))
    res = {'device': torch.cuda.get_device_name(0), 'matches': N, 'listeners': N * 22, 'bytes_per_match_counted': MATCH_BYTES,
           'roofline_bytes_per_s': ROOFLINE,
           'protocol': {'regions': a.regions, 'region_seconds': a.region_seconds, 'warmup_seconds': a.warmup, 'arms': 'alternating'}}
    times, counts = {k: [] for k, _ in arms}, {}
    for k, fn in arms:
        warm(fn, a.warmup)
        counts[k] = max(3, int(a.region_seconds / region(fn, 3)))
    for _ in range(a.regions):
        for k, fn in arms:
            warm(fn, 0.05)
            times[k].append(region(fn, counts[k]))
    for k, _ in arms:
        v = sorted(times[k])
        med = v[len(v) // 2]
        res[k] = {'us_per_call': {'median': med * 1e6, 'min': v[0] * 1e6, 'max': v[-1] * 1e6, 'regions': [x * 1e6 for x in times[k]]},
                  'calls_per_region': counts[k]}
        if k.startswith('hear_'):
            res[k]['bytes_per_s_of_the_counted_traffic'] = MATCH_BYTES * N / med
            res[k]['fraction_of_roofline'] = MATCH_BYTES * N / med / ROOFLINE
    for k in (2, 11, 22):
        eng.hear_step(says[k])
        res[f'hear_{k}']['heard_share'] = {'ours': eng.hear[:, :, 0].mean().item(), 'theirs': eng.hear[:, :, 16].mean().item()}
        res[f'hear_{k}']['over_see'] = res[f'hear_{k}']['us_per_call']['median'] / res['see']['us_per_call']['median']
        res[f'torch_{k}']['over_hear'] = res[f'torch_{k}']['us_per_call']['median'] / res[f'hear_{k}']['us_per_call']['median']
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
