"""The observation layer of the 11v11 match (relative tables, per-agent rows, see rows) in plain float64, and the rule by which an
fp32 result (a host restatement or the device) is held against it.  TEST INFRASTRUCTURE (tests/test_match_obs_f64_host.py,
tests/test_gpu_match_obs_f64.py), in the style of tests/match_f64.py.

The reference is written from the prose of include/s2d_match.h ("Per-agent relative tables", "Per-agent observations", "Vision") as
whole-array NumPy in float64: libm functions, true divisions, no fmaf order.  Its only bit-level ingredients are integers (the
Philox words of the identity bands) and parameters taken as data (every parameter rounded to fp32 once, as the engine holds them;
the kickable bound as agent_obs.params derives it).

The rule (the unit is one agent row: match, agent):
  * float64 runs from the state as given, from K_PROBES copies whose float words (x, y, vx, vy, body, neck) are moved by 1..3 fp32
    ulps in a random direction (fixed seed), and from two copies moved by 3 ulps towards and away from zero;
  * a row is ILL-CONDITIONED if any of these runs changes one of its discrete words (agent rows: is_kickable, every reach_steps,
    first / second reach and unum, the kickable unums, the integer words; see rows: level, team, unum, every quantised word, the
    order of the player rows; relative tables: nothing);
  * a well-conditioned row must reproduce every float64 discrete word exactly; a quantised see word must be the same grid point,
    |f32 - f64| <= 4 ulp of the float64 value (each word is at most two fp32 roundings of a grid point or of a product of two, and
    the coarsest rounding is 1e4 times finer than the finest grid step); +0 equals -0 and a direction of -180 equals +180;
  * a continuous word must satisfy |f32 - f64| <= T_word + 2 * spread, spread = the largest deviation of the probe runs from the
    unperturbed one, T in units of one fp32 ulp at the word's natural magnitude (UNIT);
  * the share of ill-conditioned rows is reported so that callers can cap it (ILL_CAP, EDGE_ILL_CAP for the constructed scenes).
"""
import os
import sys

import numpy as np

import agent_obs as A
import match_f64 as MF
import match_see as S
from soccer2d_amd import _capi_match as M

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
from s2d_oracle_numpy import philox4x32_10  # noqa: E402

K_PROBES, PROBE_ULPS = MF.K_PROBES, MF.PROBE_ULPS
ILL_CAP, EDGE_ILL_CAP = 0.01, 0.15
MOVED = ('x', 'y', 'vx', 'vy', 'body', 'neck')           # the float words the observations compute with
STATE_KEYS = A.OBJ_PLANES + A.ENV_WORDS + ('tick',) + S.VISION_PLANES
NONE = M.REACH_NONE
ALL = 0x3FFFFF
# one fp32 ulp at the word's natural magnitude: pitch half length, ball_speed_max, 180 degrees, the pitch diagonal, kick_power_rate
UNIT = {k: float(np.spacing(np.float32(m))) for k, m in (
    ('pos', 52.5), ('vel', 3.0), ('body', 180.0), ('neck', 180.0), ('face', 180.0), ('bearing', 180.0), ('dist', 125.0),
    ('kick_rate', 0.027), ('line', 52.5), ('rel_dist', 125.0), ('rel_angle', 180.0))}
# T_word in those units.  Measured over the CPU corpus of tests/test_match_obs_f64_host.py (the fp32 restatements against this
# reference: max over well-conditioned rows of (|f32 - f64| - 2 spread) / unit, every corpus entry); each T is at most 4x the
# measured maximum (in the comment).  A measured value <= 0 (a copy, or an error inside the spread everywhere) gives T = 0.
T_ULPS = {'pos': 0.0, 'vel': 0.0, 'neck': 0.0,           # measured <= 0: copies, the sign change of the own frame is exact
          'body': 1.4,                                   # measured 0.48 (the rounding of b -+ 180 for a right-team body)
          'face': 1.9,                                   # measured 0.48 (the rounding of body + neck, played states)
          'dist': 0.0, 'rel_dist': 0.0, 'line': 0.0,     # measured <= 0: hypot2's rounding is inside the spread; the lines are copies
          'bearing': 5.5,                                # measured 1.57
          'kick_rate': 4.0,                              # measured 1.02
          'rel_angle': 2.2}                              # measured 0.57

RIGHT = np.arange(22) >= 11
SGN = np.where(RIGHT, -1.0, 1.0)
# OWN[p][k] = the raw slot of own-frame slot k for agent p (his team 0..10 first); column 22 = the ball
OWN = np.array([[(k + 11) % 22 if p >= 11 else k for k in range(22)] + [22] for p in range(22)])
ME = np.arange(22) % 11                                 # the agent's own own-frame slot
AR = np.arange(22)
PENALTY_MODES = (22, 23, 24, 25, 26, 28, 29)
SET_PLAY_MODES = (M.GM_KICK_OFF, M.GM_KICK_IN, M.GM_FREE_KICK, M.GM_CORNER_KICK, M.GM_GOAL_KICK, M.GM_IND_FREE_KICK,
                  M.GM_GOALIE_CATCH, M.GM_PENALTY_KICK)


def _rows_of(mask):
    return [i for i in range(22) if (mask >> i) & 1]


def norm_deg(d):
    d = np.where(np.abs(d) > 360.0, np.fmod(d, 360.0), d)
    d = np.where(d < -180.0, d + 360.0, d)
    return np.where(d > 180.0, d - 360.0, d)


def atan2_deg(y, x):
    return np.where((x == 0.0) & (y == 0.0), 0.0, np.degrees(np.arctan2(y, x)))


def _f64(state, k, cols=23):
    return np.asarray(state[k], dtype=np.float64)[:, :cols]


def _side_word(side, ours):
    """+1 ours, -1 theirs, 0 none; side [n] (0 none, 1 left, 2 right), ours [22] -> [n, 22]"""
    side = np.asarray(side)[:, None]
    return np.where(side == ours[None, :], 1.0, np.where(side == 0, 0.0, -1.0))


def _turned(b):
    return np.where(b > 0.0, b - 180.0, b + 180.0)


def _own_frame(state):
    """own-frame x, y, vx, vy [n, 22 agents, 23 objects in own-frame slot order] and bodies [n, 22, 22]"""
    x, y, vx, vy = (_f64(state, k) for k in ('x', 'y', 'vx', 'vy'))
    sg = SGN[None, :, None]
    body = _f64(state, 'body', 22)
    bo = np.where(RIGHT[None, :, None], _turned(body)[:, OWN[:, :22]], body[:, OWN[:, :22]])
    return sg * x[:, OWN], sg * y[:, OWN], sg * vx[:, OWN], sg * vy[:, OWN], bo


# ------------------------------------------------------------------------------------------------ the reference
def relative(state):
    """dist, angle [n, 22, 23]: distance and absolute direction of object j seen from agent p; the diagonal is 0"""
    x, y = _f64(state, 'x'), _f64(state, 'y')
    dx, dy = x[:, None, :] - x[:, :22, None], y[:, None, :] - y[:, :22, None]
    eye = np.eye(22, 23, dtype=bool)[None]
    return np.where(eye, 0.0, np.hypot(dx, dy)), np.where(eye, 0.0, atan2_deg(dy, dx))


def cycles_to_period_end(cycle, half, total, nr_extra, extra_half):
    """cycles until the clock reaches the end of the half (or, once normal time is over and extra halves are played, the extra
    half) that `cycle` lies in; a clock standing on an end is at the start of the next period"""
    cycle = np.asarray(cycle, dtype=np.int64)
    extra = (nr_extra > 0) & (cycle >= total)
    c = np.where(extra, cycle - total, cycle)
    length = np.where(extra, max(extra_half, 1), half)
    return (c // length + 1) * length - c


def reach_steps(state, P):
    """(kickable, reach) [n, 22]: the header's reach estimate, the same in every frame"""
    x, y = _f64(state, 'x'), _f64(state, 'y')
    active = np.asarray(state['card'])[:, :22] < M.CARD_RED
    ka, ka2, speed = (np.array(v[:], dtype=np.float64) for v in (P.ka, P.ka2, P.speed_max))
    decay = float(P.ball_decay)
    px, py = x[:, :22], y[:, :22]
    cx, cy = x[:, 22].copy(), y[:, 22].copy()
    cvx, cvy = _f64(state, 'vx')[:, 22].copy(), _f64(state, 'vy')[:, 22].copy()
    kick = active & ((cx[:, None] - px) ** 2 + (cy[:, None] - py) ** 2 <= ka2[None, :])
    reach = np.where(kick, 0, NONE)
    todo = active & ~kick
    for t in range(1, M.AGENT_REACH_MAX + 1):
        cx, cy = cx + cvx, cy + cvy
        cvx, cvy = cvx * decay, cvy * decay
        r = ka + t * speed
        hit = todo & ((cx[:, None] - px) ** 2 + (cy[:, None] - py) ** 2 <= (r * r)[None, :])
        reach = np.where(hit, t, reach)
        todo &= ~hit
    return kick, reach


def _two_smallest(reach, ok):
    """reach, ok [n, 22, m] -> (first reach, first unum, second reach, second unum): the two smallest (reach, slot) keys"""
    m = reach.shape[-1]
    key = np.where(ok, reach * 64 + np.arange(m), 1 << 20)
    srt = np.sort(key, axis=-1)
    out = []
    for i in range(2):
        k = srt[..., i]
        have = k < (1 << 20)
        out += [np.where(have, k // 64, NONE), np.where(have, k % 64 + 1, 0)]
    return out


def _first_unum(flag):
    """flag [n, 22, m] -> 1 + the lowest index set, 0 if none"""
    return np.where(flag.any(axis=-1), flag.argmax(axis=-1) + 1, 0)


def agent_rows(state, cfg):
    """float64 [n, 22, 224]: the per-agent observation rows"""
    P = A.params(cfg)
    X, Y, VX, VY, B = _own_frame(state)
    n = X.shape[0]
    card = np.asarray(state['card'])[:, :22]
    active = card < M.CARD_RED
    kick, reach = reach_steps(state, P)
    act_o, kick_o, reach_o = active[:, OWN[:, :22]], kick[:, OWN[:, :22]], reach[:, OWN[:, :22]]
    xs, ys, bs = X[:, AR, ME], Y[:, AR, ME], B[:, AR, ME]
    bx, by = X[:, :, 22], Y[:, :, 22]
    o = np.zeros((n, 22, M.AGENT_OBS_DIM))
    # self
    o[..., 0], o[..., 1], o[..., 2], o[..., 3], o[..., 4] = xs, ys, VX[:, AR, ME], VY[:, AR, ME], bs
    for i, k in enumerate(('stamina', 'effort', 'recovery', 'stamina_capacity')):
        o[..., 5 + i] = _f64(state, k, 22)
    o[..., 9] = (ME == 0)[None, :]
    o[..., 10], o[..., 11] = np.asarray(state['tackle_cycles'])[:, :22], card
    bdist = np.hypot(bx - xs, by - ys)
    bbear = norm_deg(atan2_deg(by - ys, bx - xs) - bs)
    f32 = lambda v: float(np.float32(v))                                      # noqa: E731  (a parameter, rounded to fp32 once)
    types = [cfg.player_types[cfg.player_type_id[i]] for i in range(22)]
    kpr, margin, size = (np.array([f32(getattr(t, k)) for t in types]) for k in ('kick_power_rate', 'kickable_margin', 'player_size'))
    rate = kpr * (1.0 - 0.25 * (np.abs(bbear) / 180.0) - 0.25 * ((bdist - size - f32(cfg.sp.ball_size)) / margin))
    o[..., 12], o[..., 13] = kick, np.where(kick, rate, 0.0)
    o[..., 14], o[..., 15] = np.asarray(state['catch_ban'])[:, :22], np.array(P.type_id[:])[None, :]
    # ball
    ours = np.where(RIGHT, 2, 1)
    holder = np.asarray(state['ball_holder'])
    o[..., 16], o[..., 17], o[..., 18], o[..., 19], o[..., 20], o[..., 21] = bx, by, VX[:, :, 22], VY[:, :, 22], bdist, bbear
    o[..., 22] = _side_word(state['last_touch_side'], ours)
    o[..., 23] = _side_word(np.where(holder > 0, np.where(holder - 1 < 11, 1, 2), 0), ours)
    # game
    mode, mside = np.asarray(state['mode']), np.asarray(state['mode_side'])
    sl, sr = np.asarray(state['score_left'])[:, None], np.asarray(state['score_right'])[:, None]
    o[..., 24], o[..., 25] = mode[:, None], _side_word(mside, ours)
    o[..., 26], o[..., 27] = np.where(RIGHT[None], sr, sl), np.where(RIGHT[None], sl, sr)
    o[..., 28], o[..., 29] = np.asarray(state['cycle'])[:, None], np.asarray(state['stopped_cycle'])[:, None]
    o[..., 30] = cycles_to_period_end(state['cycle'], P.half_time_cycles, P.total_cycles, P.nr_extra_halfs, P.extra_half_cycles)[:, None]
    o[..., 31] = np.isin(mode, PENALTY_MODES)[:, None]
    opp_x = np.sort(X[:, :, 11:22], axis=-1)                                  # all 11 opponents, sent-off ones included
    o[..., 32] = np.maximum(0.0, np.maximum(bx, opp_x[..., -2]))              # (the second-largest counts equal values twice)
    o[..., 33] = np.minimum(bx, np.where(act_o[:, :, 1:11], X[:, :, 1:11], np.inf).min(axis=-1))
    o[..., 34] = np.maximum(bx, np.where(act_o[:, :, 12:22], X[:, :, 12:22], -np.inf).max(axis=-1))
    not_me = np.arange(11)[None, :] != ME[:, None]                            # [22, 11]
    o[..., 35] = _first_unum(kick_o[:, :, :11] & not_me[None])
    o[..., 36] = _first_unum(kick_o[:, :, 11:])
    o[..., 37] = reach
    o[..., 38], o[..., 39], o[..., 40], o[..., 41] = _two_smallest(reach_o[:, :, :11], act_o[:, :, :11] & not_me[None])
    o[..., 42], o[..., 43], o[..., 44], o[..., 45] = _two_smallest(reach_o[:, :, 11:], act_o[:, :, 11:])
    setp = np.isin(mode, SET_PLAY_MODES)[:, None]
    word = _side_word(mside, ours)
    o[..., 46], o[..., 47] = setp & (word == 1.0), setp & (word == -1.0)
    # teammates, opponents: 22 rows of 8 words in own-frame slot order
    dx, dy = X[:, :, :22] - xs[..., None], Y[:, :, :22] - ys[..., None]
    mine = (np.arange(22)[None, :] == ME[:, None])[None]
    rows = np.stack([X[:, :, :22], Y[:, :, :22], VX[:, :, :22], VY[:, :, :22], B,
                     np.where(mine, 0.0, np.hypot(dx, dy)), np.where(mine, 0.0, norm_deg(atan2_deg(dy, dx) - bs[..., None])),
                     reach_o.astype(np.float64)], axis=-1)
    rows[..., :7] = np.where(act_o[..., None], rows[..., :7], 0.0)
    o[..., 48:] = rows.reshape(n, 22, 176)
    return o


def vision_values(params):
    """S2DVisionParams (DEFAULTS overwritten with `params`) as the layer holds them: every word rounded to fp32 once"""
    v = dict(S.DEFAULTS)
    v.update(params or {})
    out = {}
    for k, x in v.items():
        out[k] = tuple(float(np.float32(a)) for a in x) if isinstance(x, (tuple, list)) else float(np.float32(x))
    return out


def identity_draws(seed, ids, tick):
    """u1, u2 [n, 22, 23] (own-frame object order): the identity bands' uniforms -- Philox stream 8, counter = tick, block = p*24+j"""
    ids = np.asarray(ids, dtype=np.uint64)
    n = len(ids)
    block = (np.arange(22)[:, None] * 24 + OWN).astype(np.uint64)             # raw slots
    c3 = np.broadcast_to((np.uint64(M.MATCH_ST_SEE) << np.uint64(16)) | block, (n, 22, 23))
    bc = lambda a: np.broadcast_to(np.asarray(a, dtype=np.uint64)[:, None, None], (n, 22, 23))   # noqa: E731
    t = (np.asarray(tick, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint64)
    w = philox4x32_10(bc(ids & np.uint64(0xFFFFFFFF)), bc(ids >> np.uint64(32)), bc(t), c3,
                      int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    u = lambda x: (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24         # noqa: E731
    return u(w[0]), u(w[1])


def _quant(v, q):
    return np.rint(v / q) * q


def see_rows(state, vision, params, seed, ids):
    """(float64 [n, 22, 192], int [n, 22, 21]): the see rows, and the own-frame slot of the player in each player row (-1: none)"""
    V = vision_values(params)
    X, Y, VX, VY, B = _own_frame(state)
    n = X.shape[0]
    card = np.asarray(state['card'])[:, :22]
    active = card < M.CARD_RED
    neck = _f64(vision, 'neck', 22)
    width = np.asarray(vision['view_width'])[:, :22]
    wait = np.asarray(vision['see_wait'])[:, :22]
    wi = np.where(width == M.VIEW_NARROW, 0, np.where(width == M.VIEW_WIDE, 2, 1))
    half_angle = 0.5 * np.array(V['view_angle'])[wi]
    fresh = wait == np.array([int(i) for i in V['see_interval']])[wi]
    xs, ys, vxs, vys, bs = X[:, AR, ME], Y[:, AR, ME], VX[:, AR, ME], VY[:, AR, ME], B[:, AR, ME]
    face = norm_deg(bs + neck)
    o = np.zeros((n, 22, M.SEE_DIM))
    for i, v in enumerate((xs, ys, vxs, vys, bs, neck, face, wi + 1, fresh, wait)):
        o[..., i] = v
    for i, k in enumerate(('stamina', 'effort', 'recovery', 'stamina_capacity')):
        o[..., 10 + i] = _f64(state, k, 22)
    o[..., 14], o[..., 15] = (ME == 0)[None, :], card
    o[..., 21] = np.asarray(state['mode'])[:, None]
    o[..., 22] = _side_word(state['mode_side'], np.where(RIGHT, 2, 1))
    o[..., 23] = np.asarray(state['cycle'])[:, None]
    # every object j (own-frame order, 22 = ball) as agent p sees it
    dx, dy = X - xs[..., None], Y - ys[..., None]
    d = np.hypot(dx, dy)
    zero = d == 0.0
    ds = np.where(zero, 1.0, d)
    rel = np.where(zero, 0.0, norm_deg(atan2_deg(dy, dx) - face[..., None]))
    in_cone = np.abs(rel) <= half_angle[..., None]
    felt = d <= V['visible_distance']
    u1, u2 = identity_draws(seed, ids, state['tick'])
    uf, utf, tf, ttf = (V[k] for k in ('unum_far_length', 'unum_too_far_length', 'team_far_length', 'team_too_far_length'))
    p1 = (d - uf) / (utf - uf) if utf > uf else np.full_like(d, np.inf)
    p2 = (d - tf) / (ttf - tf) if ttf > tf else np.full_like(d, np.inf)
    by_dist = np.where(d <= uf, 4, np.where((d < utf) & (u1 >= p1), 4, np.where(d <= tf, 3, np.where((d < ttf) & (u2 >= p2), 3, 2))))
    is_ball = (np.arange(23) == 22)[None, None, :]
    level = np.where(in_cone, np.where(is_ball, 4, by_dist), np.where(felt, 1, 0))
    other = np.arange(23)[None, :] != ME[:, None]                             # [22, 23]
    obj_active = np.concatenate([active[:, OWN[:, :22]], np.ones((n, 22, 1), bool)], axis=2)
    level = np.where((fresh & active)[..., None] & other[None] & obj_active, level, 0)
    seen, full = level >= 1, level == 4
    dist = np.where(seen & ~zero, _quant(np.exp(_quant(np.log(ds), V['dist_quantize_step'])), V['dist_round']), 0.0)
    direc = np.where(seen, np.rint(rel), 0.0)
    ex, ey = dx / ds, dy / ds
    rvx, rvy = VX - vxs[..., None], VY - vys[..., None]
    moving = full & ~zero
    dist_chg = np.where(moving, dist * _quant((rvx * ex + rvy * ey) / ds, V['dist_chg_quantize']), 0.0)
    dir_chg = np.where(moving, _quant(((rvy * ex - rvx * ey) / ds) * (180.0 / np.pi), V['dir_chg_quantize']), 0.0)
    o[..., 16], o[..., 17], o[..., 18], o[..., 19], o[..., 20] = level[..., 22], dist[..., 22], direc[..., 22], dist_chg[..., 22], dir_chg[..., 22]
    # the player rows: seen ones first, ascending by (dir, dist, own-frame slot)
    k = np.arange(22)[None, None, :]
    lv, sn, fl = level[..., :22], seen[..., :22], full[..., :22]
    rows = np.stack([lv, np.where(lv >= 3, np.where(k < 11, 1.0, -1.0), 0.0), np.where(fl, k % 11 + 1, 0), dist[..., :22], direc[..., :22],
                     dist_chg[..., :22], dir_chg[..., :22], np.where(fl, np.rint(norm_deg(B - face[..., None])), 0.0)], axis=-1).astype(np.float64)
    by_d = np.argsort(np.where(sn, dist[..., :22], np.inf), axis=-1, kind='stable')
    dir_key = np.take_along_axis(np.where(sn, direc[..., :22], np.inf), by_d, axis=-1)
    order = np.take_along_axis(by_d, np.argsort(dir_key, axis=-1, kind='stable'), axis=-1)      # [n, 22, 22]; the agent himself is unseen
    rows = np.take_along_axis(rows, order[..., None], axis=2)[:, :, :21]
    o[..., 24:] = rows.reshape(n, 22, 168)
    slot = np.where(np.take_along_axis(sn, order, axis=-1), order, -1)[:, :, :21]
    return o, slot


# ------------------------------------------------------------------------------------------------ the rule
def perturb(state, rs, ulps=PROBE_ULPS, scale=0):
    """match_f64.perturb's scheme on the words the observations read: a copy of `state` with x, y, vx, vy, body (23 objects) and neck
    moved by 1..ulps fp32 ulps in a random direction; scale = -1 / +1: every word moved by `ulps` ulps towards / away from zero"""
    out = dict(state)
    for f in MOVED:
        if f not in state:
            continue
        full = np.array(state[f], dtype=np.float32)
        v = full[:, :23]
        if scale:
            steps = np.where(v < 0, -1, 1) * scale * ulps
        else:
            steps = rs.randint(1, ulps + 1, size=v.shape) * rs.choice([-1, 1], size=v.shape)
        for k in range(ulps):
            move = np.abs(steps) > k
            v = np.where(move, np.nextafter(v, np.where(steps > 0, np.float32(np.inf), np.float32(-np.inf))), v)
        full[:, :23] = v
        out[f] = full
    return out


class Words:
    """how each word of a row is compared: kind 0 = discrete (exact), 1 = continuous (T name), 2 = quantised; circ = a direction"""

    def __init__(self, dim):
        self.kind = np.zeros(dim, dtype=np.int8)
        self.circ = np.zeros(dim, dtype=bool)
        self.name = [None] * dim

    def cont(self, idx, name, circ=False):
        for i in np.atleast_1d(np.arange(len(self.kind))[idx]):
            self.kind[i], self.circ[i], self.name[i] = 1, circ, name

    def quant(self, idx, circ=False):
        for i in np.atleast_1d(np.arange(len(self.kind))[idx]):
            self.kind[i], self.circ[i] = 2, circ


def _agent_words():
    w = Words(M.AGENT_OBS_DIM)
    for base in (0, 16):
        w.cont(slice(base, base + 2), 'pos'); w.cont(slice(base + 2, base + 4), 'vel')
    w.cont(4, 'body', True); w.cont(13, 'kick_rate'); w.cont(20, 'dist'); w.cont(21, 'bearing', True)
    w.cont(slice(32, 35), 'line')
    for r in range(22):
        b = 48 + 8 * r
        w.cont(slice(b, b + 2), 'pos'); w.cont(slice(b + 2, b + 4), 'vel'); w.cont(b + 4, 'body', True)
        w.cont(b + 5, 'dist'); w.cont(b + 6, 'bearing', True)
    return w


def _see_words():
    w = Words(M.SEE_DIM)
    w.cont(slice(0, 2), 'pos'); w.cont(slice(2, 4), 'vel'); w.cont(4, 'body', True); w.cont(5, 'neck', True); w.cont(6, 'face', True)
    w.quant(17); w.quant(18, True); w.quant(19); w.quant(20)
    for r in range(21):
        b = 24 + 8 * r
        w.quant(b + 3); w.quant(b + 4, True); w.quant(b + 5); w.quant(b + 6); w.quant(b + 7, True)
    return w


def _rel_words():
    w = Words(46)
    w.cont(slice(0, 23), 'rel_dist'); w.cont(slice(23, 46), 'rel_angle', True)
    return w


AGENT_WORDS, SEE_WORDS, REL_WORDS = _agent_words(), _see_words(), _rel_words()


def _diff(a, b, circ):
    d = np.abs(a - b)
    return np.where(circ, np.minimum(d, np.abs(360.0 - d)), d)


def _same_grid(a, b, circ):
    """a is the grid point b: within 4 fp32 ulps of b (+0 == -0, and for a direction -180 == +180)"""
    return _diff(a, b, circ) <= 4.0 * np.spacing(np.abs(b).astype(np.float32)).astype(np.float64) * (b != 0.0)


def _compare(words, fn, state, got, rows, T, seed, probes, extra=None):
    """fn(state) -> float64 [n, 22, dim] (with `extra`: and an array [n, 22, m] of discrete words that the probes watch but the row
    does not hold, the slot order of a see row); got: fp32 [n, len(rows), dim]"""
    res = fn(state)
    base, base_x = (res, None) if extra is None else res
    base = base[:, rows]
    di, ci, qi = (np.flatnonzero(words.kind == k) for k in (0, 1, 2))
    cc, qc = words.circ[ci][None, None, :], words.circ[qi][None, None, :]
    ill = np.zeros(base.shape[:2], dtype=bool)
    spread = np.zeros(base.shape[:2] + (len(ci),))
    rs = np.random.RandomState(seed)
    for k in range(probes + 2):
        scale = 0 if k < probes else (-1 if k == probes else 1)
        res = fn(perturb(state, rs, scale=scale))
        p, p_x = (res, None) if extra is None else res
        p = p[:, rows]
        ill |= (p[..., di] != base[..., di]).any(axis=-1)
        if len(qi):
            ill |= (~_same_grid(p[..., qi], base[..., qi], qc)).any(axis=-1)
        if p_x is not None:
            ill |= (p_x[:, rows] != base_x[:, rows]).any(axis=-1)
        spread = np.maximum(spread, _diff(p[..., ci], base[..., ci], cc))
    well = ~ill
    fails = []
    g = np.asarray(got, dtype=np.float64)
    assert g.shape == base.shape, (g.shape, base.shape)

    def report(bad, cols, what):
        idx = np.argwhere(bad & well[..., None])
        if len(idx):
            e, r, w = idx[0]
            w = cols[w]
            fails.append(f'{what}: {len(idx)} words of well-conditioned rows differ; match {e} agent {rows[r]} word {w}: '
                         f'f32={float(g[e, r, w])!r} f64={float(base[e, r, w])!r}')
    report(g[..., di] != base[..., di], di, 'discrete')
    if len(qi):
        report(~_same_grid(g[..., qi], base[..., qi], qc), qi, 'quantised')
    err = _diff(g[..., ci], base[..., ci], cc)
    names = [words.name[i] for i in ci]
    worst = {}
    for name in sorted(set(names)):
        sel = np.array([nm == name for nm in names])
        excess = (err[..., sel] - 2.0 * spread[..., sel]) / UNIT[name]
        excess = np.where(well[..., None], excess, -np.inf)
        worst[name] = float(excess.max()) if excess.size else -np.inf
        if T is not None and worst[name] > T[name]:
            e, r, w = np.unravel_index(np.argmax(excess), excess.shape)
            c = np.flatnonzero(sel)[w]
            w = ci[c]
            fails.append(f'{name}: |f32 - f64| - 2 spread = {worst[name]:.2f} ulps > {T[name]} at match {e} agent {rows[r]} word {w}: '
                         f'f32={float(g[e, r, w])!r} f64={float(base[e, r, w])!r} spread={float(spread[e, r, c])!r}')
    n_rows = int(well.size)
    return dict(n=n_rows, ill=int(ill.sum()), share=float(ill.sum()) / max(n_rows, 1), well=well, worst=worst, f64=base,
                spread=spread, cont_words=ci), fails


def compare_agent(state, cfg, got, mask=ALL, T=T_ULPS, seed=0x0B5, probes=K_PROBES):
    """(report, failures) of fp32 agent rows `got` [n, popcount(mask), 224] against float64"""
    return _compare(AGENT_WORDS, lambda s: agent_rows(s, cfg), state, got, _rows_of(mask), T, seed, probes)


def compare_see(state, params, seed_philox, ids, got, mask=ALL, T=T_ULPS, seed=0x5EE, probes=K_PROBES):
    """(report, failures) of fp32 see rows `got` [n, popcount(mask), 192] against float64.  The vision planes are part of `state`.
    The probes watch the order of the player rows as the float64 slot order; an fp32 row does not name slots: it shows its order
    through every word standing in the right row (the constructed scenes tell equal keys apart by unum)."""
    def fn(s):
        return see_rows(s, s, params, seed_philox, ids)
    return _compare(SEE_WORDS, fn, state, got, _rows_of(mask), T, seed, probes, extra=True)


def bearings(state):
    """float64 [n, 22, 23]: direction of object j seen from agent p relative to p's body (absolute frame; the diagonal is 0): what
    MatchEngine.egocentric_tables returns, and -- the own frame turns both terms by 180 degrees -- the agent rows' bearing words"""
    _, angle = relative(state)
    return np.where(np.eye(22, 23, dtype=bool)[None], 0.0, norm_deg(angle - _f64(state, 'body', 22)[:, :, None]))


def compare_bearings(state, got, T=T_ULPS, seed=0xBEA, probes=K_PROBES):
    """(report, failures) of fp32 bearings [n, 22, 23] against float64; the unit is one agent's 23 cells"""
    w = Words(23)
    w.cont(slice(0, 23), 'bearing', True)
    return _compare(w, bearings, state, got, list(range(22)), T, seed, probes)


def row_bearings(agent):
    """[n, 22, 23]: the bearing words of full-mask agent rows, indexed by raw object (players' rows, then the ball's word)"""
    agent = np.asarray(agent)
    out = np.zeros(agent.shape[:2] + (23,), dtype=agent.dtype)
    for p in range(22):
        out[:, p, OWN[p, :22]] = agent[:, p, 48 + 6:224:8]
        out[:, p, 22] = agent[:, p, 21]
    return out


def compare_relative(state, dist, angle, T=T_ULPS, seed=0x4E1, probes=K_PROBES):
    """(report, failures) of fp32 relative tables [n, 22, 23] against float64; the unit is one agent's 23 cells"""
    def fn(s):
        return np.concatenate(relative(s), axis=-1)
    got = np.concatenate([np.asarray(dist), np.asarray(angle)], axis=-1)
    return _compare(REL_WORDS, fn, state, got, list(range(22)), T, seed, probes)


# ------------------------------------------------------------------------------------------------ states
def random_state(rng, n, vision_params=None):
    """agent_obs.random_state with ticks and random vision planes: every word the three kernels read"""
    s = A.random_state(rng, n)
    s['tick'] = rng.integers(0, 20000, n).astype(np.int32)
    s.update(S.random_vision(rng, n, S.params(**(vision_params or {}))))
    return s


def mirror(state):
    """the mirrored state (agent_obs.mirror); ticks stay, each player's vision words move with him"""
    perm = np.r_[11:22, 0:11, 22, 23]
    m = A.mirror(state)
    m['tick'] = np.asarray(state['tick']).copy()
    for k in S.VISION_PLANES:
        m[k] = np.asarray(state[k])[:, perm].copy()
    return m


# ------------------------------------------------------------------------------------------------ constructed edge scenes
LEVEL, TEAM, UNUM, DIST, DIR, DIST_CHG, DIR_CHG, BODY_REL = range(8)     # words of one player row of a see row


def prow(r, w):
    """index of word w of player row r in a see row"""
    return 24 + 8 * r + w


def edge_scenes(cfg, vision_params=None):
    """(state, known): one small batch of constructed scenes, each built once for a left agent (slot 5) and once for a right agent
    (slot 16) in that agent's own frame, and the known answers the header fixes: a list of (scene, kind, match, agent, word, op,
    value) with kind 'agent' | 'see' | 'dist' | 'angle' (relative tables: word = object) and op 'eq' | 'abs' (|word| == value) |
    'ge' | 'near' (within 1e-4).

    The base of every scene: each team on its own goal line side (own-frame x = -50, y = -30 + 6 k), at rest, looking away from
    the pitch, normal width, fresh; the ball at rest at the centre.  Nobody sees or feels anything until a scene moves someone."""
    V = vision_values(vision_params)
    P = A.params(cfg)
    f32 = np.float32
    up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))                  # noqa: E731
    dn = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))                 # noqa: E731
    scenes, known = [], []

    class Scene:
        def __init__(self, name, side):
            self.name, self.side, self.e = f'{name} ({"left" if side > 0 else "right"})', side, len(scenes)
            s = {k: np.zeros((1, 24), dtype=np.float32 if k in A.FLOAT_PLANES else np.int32) for k in A.OBJ_PLANES}
            s.update({k: np.zeros((1,), dtype=np.int32) for k in A.ENV_WORDS + ('tick',)})
            s['neck'] = np.zeros((1, 24), dtype=np.float32)
            s['view_width'] = np.full((1, 24), 2, dtype=np.int32)
            s['see_wait'] = np.full((1, 24), int(V['see_interval'][1]), dtype=np.int32)
            s['stamina'][:, :22], s['effort'][:, :22], s['recovery'][:, :22], s['stamina_capacity'][:, :22] = 8000.0, 1.0, 1.0, 130600.0
            s['mode'][:], s['tick'][:], s['cycle'][:] = M.GM_PLAY_ON, 77 + len(scenes), 100
            self.s = s
            self.agent = self.raw(5)
            for k in range(22):
                self.put(k, -50.0 if k < 11 else 50.0, -30.0 + 6.0 * (k % 11), body=180.0 if k < 11 else 0.0)
            scenes.append(self)

        def raw(self, k):
            return k if k == 22 or self.side > 0 else (k + 11) % 22

        def put(self, k, x, y, vx=0.0, vy=0.0, body=None, **words):
            """own-frame slot k (22 = the ball) at own-frame (x, y), velocity and body"""
            j, sg = self.raw(k), f32(self.side)
            for name, v in (('x', x), ('y', y), ('vx', vx), ('vy', vy)):
                self.s[name][0, j] = sg * f32(v)
            if body is not None:
                b = f32(body)
                self.s['body'][0, j] = b if self.side > 0 else (b - f32(180.0) if b > 0 else b + f32(180.0))
            for name, v in words.items():
                self.s[name][0, j] = v

        def me(self, x=0.0, y=0.0, body=0.0, neck=0.0, width=2, wait=None, park='behind', **kw):
            """the scene's agent (own-frame slot 5); everybody else is parked on an arc of 60 m radius behind his back (or in front
            of his face), 3 degrees apart, looking outwards: out of his view, and out of each other's reach"""
            w = width if width in (1, 2, 3) else 2
            self.put(5, x, y, body=body, neck=neck, view_width=width,
                     see_wait=int(V['see_interval'][w - 1]) if wait is None else wait, **kw)
            step = max(3.0, float(np.degrees(1.2 * V['visible_distance'] / 60.0)))      # neighbours do not feel each other
            norm = lambda a: a - 360.0 * np.floor((a + 180.0) / 360.0)                    # noqa: E731
            for k in range(22):
                if k != 5:
                    a = norm(body + neck + (180.0 if park == 'behind' else 0.0) + step * (k - 10.5))
                    self.put(k, x + 60.0 * np.cos(np.radians(a)), y + 60.0 * np.sin(np.radians(a)), body=norm(a + 7.3))

        def know(self, kind, word, value, op='eq', agent=None):
            known.append((self.name, kind, self.e, self.agent if agent is None else self.raw(agent), word, op, value))

    def both(name):
        return [Scene(name, +1), Scene(name, -1)]

    F_ = M.AGENT_OBS_FIELDS
    # ---- distance and direction
    for sc in both('ball on the agent: d == 0'):
        sc.me(); sc.put(22, 0.0, 0.0, 0.5, 0.5)
        for w, v in ((16, 4), (17, 0), (18, 0), (19, 0), (20, 0)):
            sc.know('see', w, v)
        sc.put(12, 0.0, 0.0, -0.5, 0.25, body=90.0)                          # an opponent on the same point: level 4, body_rel carried
        for w, v in ((LEVEL, 4), (TEAM, -1), (UNUM, 2), (DIST, 0), (DIR, 0), (DIST_CHG, 0), (DIR_CHG, 0), (BODY_REL, 90)):
            sc.know('see', prow(0, w), v)
    for d in (1e-6, 1e-3):
        for sc in both(f'ball {d} m ahead'):                                  # log(d) / 0.1 -> exp -> / 0.1 rounds to 0: dist = 0
            sc.me(); sc.put(22, d, 0.0, -0.5, 0.25)
            sc.know('see', 16, 4); sc.know('see', 18, 0)
            if vision_params is None:
                sc.know('see', 17, 0); sc.know('see', 19, 0)                  # dist_chg = 0 * (a negative grid point) = -0
    vd = V['visible_distance']
    for tag, d, lvl in (('exactly', vd, 1), ('one ulp inside', dn(vd), 1), ('one ulp outside', up(vd), 0)):
        for sc in both(f'visible_distance {tag}, outside the cone'):
            sc.me(); sc.put(22, 0.0, d); sc.put(12, 0.0, -d)                  # rel = +-90 against a half angle of 60
            sc.know('see', 16, lvl); sc.know('see', prow(0, LEVEL), lvl)
            if lvl:
                sc.know('see', 18, 90); sc.know('see', prow(0, DIR), -90)
                sc.know('see', prow(0, TEAM), 0); sc.know('see', prow(0, UNUM), 0); sc.know('see', 19, 0)
    uf, utf, tf, ttf = (V[k] for k in ('unum_far_length', 'unum_too_far_length', 'team_far_length', 'team_too_far_length'))
    fixed = {uf: 4, tf: 3 if tf >= utf else None, ttf: 2}                    # exactly on a length (the draws cannot matter there)
    if utf <= tf:
        fixed[utf] = 3
    for length in sorted({uf, utf, tf, ttf}):
        for tag, d in (('exactly', length), ('one ulp inside', dn(length)), ('one ulp outside', up(length))):
            for sc in both(f'player at {length} m {tag}'):
                sc.me(); sc.put(12, d, 0.0, 0.3, -0.2, body=45.0)
                if tag == 'exactly' and fixed.get(length) is not None:
                    lvl = fixed[length]
                    sc.know('see', prow(0, LEVEL), lvl)
                    sc.know('see', prow(0, TEAM), -1 if lvl >= 3 else 0); sc.know('see', prow(0, UNUM), 2 if lvl == 4 else 0)
                    sc.know('see', prow(0, BODY_REL), 45 if lvl == 4 else 0)
    for width in (1, 2, 3):
        half = 0.5 * V['view_angle'][width - 1]
        for tag, body, lvl in (('on the left edge', half, 4), ('on the right edge', -half, 4), ('one ulp outside the left edge', up(half), 0),
                               ('one ulp outside the right edge', dn(-half), 0)):
            if half >= 180.0:
                continue
            for sc in both(f'width {width}: ball {tag}'):                     # the ball straight along +x, the face turned by the neck
                sc.me(neck=body, width=width); sc.put(22, 10.0, 0.0)
                sc.know('see', 16, lvl); sc.know('see', 7, width)
                if lvl:
                    sc.know('see', 18, -np.rint(body))
    for sgn in (1.0, -1.0):
        for sc in both(f'face exactly {180 * sgn:+.0f}: rel wraps'):
            sc.me(body=90.0 * sgn, neck=90.0 * sgn)
            sc.put(22, -5.0, -1.0 * sgn); sc.put(12, -5.0, 1.0 * sgn); sc.put(13, -7.0, 0.0)
            sc.know('see', 6, 180.0, 'abs'); sc.know('see', 18, 11 * sgn)
            r12 = 0 if sgn > 0 else 1                                         # dirs -11, 0 (face +180) and 0, 11 (face -180)
            sc.know('see', prow(r12, DIR), -11 * sgn); sc.know('see', prow(r12, UNUM), 2)
            sc.know('see', prow(1 - r12, DIR), 0); sc.know('see', prow(1 - r12, UNUM), 3)
    for zero in (0.0, -0.0):
        for sc in both(f'straight behind, y = {zero!r}'):
            sc.me(); sc.put(22, -2.0, zero); sc.put(12, -2.5, zero)
            sc.know('see', 16, 1); sc.know('see', 18, 180, 'abs'); sc.know('see', prow(0, LEVEL), 1); sc.know('see', prow(0, DIR), 180, 'abs')
    # ---- order
    for sc in both('two players with equal (dir, dist)'):
        sc.me(); sc.put(15, 10.0, 0.0); sc.put(3, 10.0, 0.0)
        for r, (t, u) in enumerate(((1, 4), (-1, 5))):
            sc.know('see', prow(r, TEAM), t); sc.know('see', prow(r, UNUM), u)
        sc.know('see', prow(2, LEVEL), 0)
    for sc in both('three players with equal (dir, dist)'):
        sc.me(); sc.put(18, 12.0, 0.0); sc.put(2, 12.0, 0.0); sc.put(13, 12.0, 0.0)
        for r, (t, u) in enumerate(((1, 3), (-1, 3), (-1, 8))):
            sc.know('see', prow(r, TEAM), t); sc.know('see', prow(r, UNUM), u)
    for sc in both('seen and unseen interleaved by slot'):
        sc.me()
        ks = (1, 3, 7, 9, 12, 14, 18, 20)                                     # dir = (11 - k) * 4: descending in the slot
        for k in ks:
            a = np.radians((11 - k) * 4.0)
            sc.put(k, 10.0 * np.cos(a), 10.0 * np.sin(a))
        for r, k in enumerate(reversed(ks)):
            sc.know('see', prow(r, DIR), (11 - k) * 4); sc.know('see', prow(r, TEAM), 1 if k < 11 else -1)
            sc.know('see', prow(r, UNUM), k % 11 + 1)
        sc.know('see', prow(len(ks), LEVEL), 0)
    for sc in both('all 21 seen'):
        sc.me(width=3, park='front'); sc.put(22, 10.0, 1.0)
        sc.know('see', prow(20, LEVEL), 2, 'ge'); sc.know('see', 16, 4)
    for sc in both('none seen'):
        sc.me(); sc.put(22, -10.0, 0.0)
        sc.know('see', prow(0, LEVEL), 0); sc.know('see', 16, 0); sc.know('see', 8, 1)
    # ---- who sees and who is seen
    for sc in both('agent not fresh'):
        sc.me(wait=int(V['see_interval'][1]) - 1 if V['see_interval'][1] > 1 else 0); sc.put(22, 5.0, 0.0)
        sc.know('see', 8, 0); sc.know('see', 16, 0); sc.know('see', 17, 0)
    for sc in both('agent sent off'):
        sc.me(card=M.CARD_RED); sc.put(22, 5.0, 0.0); sc.put(12, 6.0, 1.0)
        sc.know('see', 15, M.CARD_RED); sc.know('see', 16, 0); sc.know('see', prow(0, LEVEL), 0)
        sc.know('agent', F_['self.is_kickable'], 0); sc.know('agent', F_['game.self_reach_steps'], NONE)
    for sc in both('a sent-off object'):
        sc.me(); sc.put(12, 5.0, 0.0, card=M.CARD_RED); sc.put(22, 6.0, 0.0)
        sc.know('see', 16, 4); sc.know('see', prow(0, LEVEL), 0)
    for width in (0, 7, -1):
        for sc in both(f'view-width word {width}'):                           # reads as normal: 45 degrees off is inside its cone
            sc.me(width=width); sc.put(22, 5.0, 5.0)
            sc.know('see', 7, 2); sc.know('see', 8, 1); sc.know('see', 16, 4 if V['view_angle'][1] >= 90.0 + 1e-3 else None)
    # ---- agent rows
    for side in (+1, -1):
        j = 5 if side > 0 else 16
        ka2, found = float(P.ka2[j]), None
        for dy in (0.0, 0.25, 0.5, 0.75):
            x0 = f32(np.sqrt(ka2 - dy * dy))
            for step in range(-8, 9):
                x = x0
                for _ in range(abs(step)):
                    x = np.nextafter(x, f32(np.inf if step > 0 else -np.inf))
                xo, y = np.nextafter(x, f32(np.inf)), f32(dy)
                sq32 = lambda a: f32(np.float64(a) * np.float64(a) + np.float64(f32(y * y)))      # noqa: E731  fmaf(a, a, y * y)
                sq64 = lambda a: float(a) ** 2 + float(y) ** 2                                    # noqa: E731
                if sq32(x) <= ka2 and sq64(x) <= ka2 and sq32(xo) > ka2 and sq64(xo) > ka2:
                    found = (float(x), float(xo), float(y))
                    break
            if found:
                break
        assert found, 'no point on the kickable bound on which fp32 and float64 agree'
        for tag, bx, kick in (('on the kickable bound', found[0], 1), ('one ulp outside the kickable bound', found[1], 0)):
            sc = Scene(f'ball {tag}', side)
            sc.me(); sc.put(22, bx, found[2])
            sc.know('agent', F_['self.is_kickable'], kick); sc.know('agent', F_['game.self_reach_steps'], 0 if kick else 1)
            sc.know('agent', 48 + 8 * 5 + 7, 0 if kick else 1)
        ka, sp = float(P.ka[j]), float(P.speed_max[j])
        for t, d in ((1, ka + 0.5 * sp), (50, ka + 49.5 * sp), (NONE, ka + 50.5 * sp)):
            sc = Scene(f'reach {t}', side)
            sc.me(x=d); sc.put(22, 0.0, 0.0)
            sc.know('agent', F_['game.self_reach_steps'], t); sc.know('agent', 48 + 8 * 5 + 7, t)
            sc.know('agent', 136 + 8 * 5 + 7, t, agent=12)                   # an opponent reads the same number in his opponents block
        sc = Scene('equal reach keys', side)
        for k, sx, sy in ((7, 1, 0), (4, -1, 0), (17, 0, 1), (13, 0, -1)):
            r = float(P.ka[sc.raw(k)]) + 2.5 * float(P.speed_max[sc.raw(k)])
            sc.put(k, sx * r, sy * r)
        for name, v in (('first_teammate_reach_steps', 3), ('first_teammate_unum', 5), ('second_teammate_reach_steps', 3),
                        ('second_teammate_unum', 8), ('first_opponent_reach_steps', 3), ('first_opponent_unum', 3),
                        ('second_opponent_reach_steps', 3), ('second_opponent_unum', 7)):
            sc.know('agent', F_['game.' + name], v)
        sc.know('agent', F_['game.first_teammate_unum'], 8, agent=4)         # self is excluded from his own teammates
        sc = Scene('two opponents with equal x on the offside line', side)
        for k, x in zip(range(11, 22), (10.0, 30.0, 30.0, 20.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0)):
            sc.put(k, x, -30.0 + 6.0 * (k - 11))
        sc.know('agent', F_['game.offside_line_x'], 30.0)
        for x_off in (0.0, 3.0):
            sc = Scene(f'a sent-off opponent parked at x = {x_off} decides the offside line', side)
            for k in range(11, 22):
                sc.put(k, -20.0, -30.0 + 6.0 * (k - 11))
            sc.put(11, 10.0, 0.0); sc.put(14, x_off, 34.0, card=M.CARD_RED); sc.put(22, -5.0, 0.0)
            sc.know('agent', F_['game.offside_line_x'], x_off)
        sc = Scene('goalie and sent-off players excluded from the defence lines', side)
        sc.put(0, -52.0, 0.0); sc.put(1, -48.0, 3.0, card=M.CARD_RED); sc.put(11, 52.0, 0.0); sc.put(12, 48.0, 3.0, card=M.CARD_RED)
        for k in range(2, 11):
            sc.put(k, -40.0 + (k - 2), 5.0 * k); sc.put(k + 11, 40.0 - (k - 2), 5.0 * k)
        sc.put(22, -10.0, 0.0)
        sc.know('agent', F_['game.our_defense_line_x'], -40.0); sc.know('agent', F_['game.their_defense_line_x'], 40.0)
        h, total, ne, eh = P.half_time_cycles, P.total_cycles, P.nr_extra_halfs, P.extra_half_cycles
        clocks = [(h - 1, 1), (h, h), (total - 1, 1), (total, eh if ne > 0 else h)]
        if ne > 0:
            clocks += [(total + eh - 1, 1), (total + eh, eh), (total + 2 * eh - 1, 1)]
        for c, want in clocks:
            sc = Scene(f'clock at {c}', side)
            sc.s['cycle'][:] = c
            sc.know('agent', F_['game.cycles_to_period_end'], want); sc.know('agent', F_['game.cycle'], c)
        for mode in range(22, 30):
            sc = Scene(f'mode {mode}', side)
            sc.s['mode'][:], sc.s['mode_side'][:] = mode, 1 + mode % 2
            sc.know('agent', F_['game.is_penalty_kick_mode'], 0 if mode == 27 else 1)
            sc.know('agent', F_['game.is_our_set_play'], 0); sc.know('agent', F_['game.game_mode_type'], mode)
    # ---- relative tables (absolute frame): coincident, axes, diagonals, 1e-6 m to the pitch diagonal
    sc = Scene('relative tables', +1)
    sc.put(5, 0.0, 0.0)
    spots = {6: (0.0, 0.0, 0.0, 0.0), 7: (1e-6, 0.0, 1e-6, 0.0), 8: (0.0, 1e-3, 1e-3, 90.0), 9: (-1.0, 0.0, 1.0, 180.0),
             10: (0.0, -10.0, 10.0, -90.0), 11: (2.0, 2.0, None, 45.0), 12: (-3.0, 3.0, None, 135.0), 13: (-4.0, -4.0, None, -135.0),
             14: (5.0, -5.0, None, -45.0), 15: (3.0, 4.0, 5.0, None), 22: (-30.0, 40.0, 50.0, None)}
    for j, (x, y, d, a) in spots.items():
        sc.put(j, x, y)
        if d is not None:
            sc.know('dist', j, float(f32(d)), 'near')
        if a is not None:
            sc.know('angle', j, a, 'near')
    sc.put(0, -52.5, -34.0); sc.put(21, 52.5, 34.0)
    sc.know('dist', 21, float(np.hypot(105.0, 68.0)), 'near', agent=0); sc.know('dist', 5, 0.0); sc.know('angle', 5, 0.0)
    sc.know('dist', 6, 0.0, agent=5); sc.know('dist', 5, 0.0, agent=6)
    state = {k: np.concatenate([s.s[k] for s in scenes]) for k in scenes[0].s}
    return state, [k for k in known if k[6] is not None]


def check_known(known, agent=None, see=None, dist=None, angle=None):
    """the known answers of edge_scenes against full-mask rows (any of them may be None): a list of failure strings"""
    have = dict(agent=agent, see=see, dist=dist, angle=angle)
    fails = []
    for name, kind, e, p, w, op, want in known:
        if have[kind] is None:
            continue
        v = float(have[kind][e, p, w])
        ok = {'eq': v == want, 'abs': abs(v) == want, 'ge': v >= want, 'near': abs(v - want) <= 1e-4}[op]
        if not ok:
            fails.append(f'{name}: {kind} row of agent {p}, word {w}: {v!r}, expected {op} {want!r}')
    return fails
