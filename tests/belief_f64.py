"""One update of the belief layer (include/s2d_match.h, "Belief") in plain float64, and the rule by which an fp32 result (the host
restatement tests/belief_ref.c or the device) is held against it.  TEST INFRASTRUCTURE (tests/test_belief_f64_host.py,
tests/test_gpu_match_belief_f64.py, tests/test_gpu_match_belief_edges.py), in the style of tests/obs_f64.py.

The reference is written from the five steps of the header's prose as whole-array NumPy in float64: libm sin / cos / atan2 / hypot,
true products and sums, no fmaf order, no fp32 rounding of face + dir.  Its only bit-level ingredients are data: every parameter
rounded to fp32 once (`values`), and the degree-to-radian factor of the level-4 velocity, which the header spells as the fp32
constant 0.017453292519943295f.  The sine and cosine take the quadrant out first (q = rint(th / 90), libm on th - 90 q in
[-45, 45]), so that they are exact at multiples of 90 degrees as DESIGN.md section 4 requires of sincos_deg.  Counts and the reset
flag are integer logic (whole numbers and halves are exact in either format).

The unit is one update of one agent row: (belief row as given in fp32, see row, flag, u) -> belief row.

The rule:
  * float64 runs from the inputs as given and from K_PROBES copies whose finite continuous input words (the belief's x, y, vx, vy;
    the see row's self x, y, vx, vy and face; every sighting's dist, dir, dist_chg, dir_chg and body_rel) are moved by 1..3 fp32
    ulps in a random direction (fixed seed);
  * a row is ILL-CONDITIONED if any probe changes a discrete outcome: which entry each level 1-3 sighting went to (or that it was
    dropped), which entries the ghost rule forgot, any count, whether an entry is known;
  * on a well-conditioned row every count must equal float64's exactly, an unknown entry must be the canonical one (all +0), and
    the copied self and game words are the see row's bit for bit (on every row, ill-conditioned or not);
  * x, y, vx, vy and body must satisfy |f32 - f64| <= T_word * UNIT_word + 2 * spread, spread = the largest deviation of the probe
    runs from the unperturbed one; body is compared on the circle (-180 == +180); two NaNs, or two equal infinities, agree;
  * the share of ill-conditioned rows is reported so that callers can cap it (ILL_CAP, EDGE_ILL_CAP for the constructed scenes).
"""
import numpy as np

import belief as B
import match_f64 as MF

K_PROBES, PROBE_ULPS = MF.K_PROBES, MF.PROBE_ULPS
ILL_CAP, EDGE_ILL_CAP = 0.01, 0.15                       # tests/obs_f64.py's
CARD_RED = 2.0                                           # S2D_CARD_RED
DEG2RAD_F32 = float(np.float32(0.017453292519943295))    # the header's constant, as data
# one fp32 ulp at the word's natural magnitude: pitch half length, ball_speed_max, 180 degrees (tests/obs_f64.py's)
UNIT = {'pos': float(np.spacing(np.float32(52.5))), 'vel': float(np.spacing(np.float32(3.0))),
        'body': float(np.spacing(np.float32(180.0)))}

# T_word, in those units: DERIVED, not measured.  The domain (every generator and scene of the tests that go through the rule keeps
# to it, `in_domain` checks it): dist <= DIST_MAX = 128 m, |x|, |y| < 128 m for every position read or written,
# |dist_chg| <= SPEED_MAX and |dir_chg * pi / 180 * dist| <= SPEED_MAX = 8 m per cycle, |face + dir| <= 360 and
# |body_rel + face| <= 360.  With e32 = 2^-24 (half an ulp, relative), DESIGN.md section 4's sincos_deg <= 2.5e-7 (absolute, on
# the sine and on the cosine) and atan2_deg <= 3e-5 degrees (which enters no continuous word: it decides ghosts only):
#   pos   X = fmaf(dist, c, sx).  (a) th = fl(face + dir) is one rounding float64 does not make: half an ulp of [256, 512) degrees
#         = 2^-16 deg = 2.663e-7 rad, a displacement of dist * 2.663e-7; norm_deg_any is exact (th -+ 360 of two multiples of
#         2^-16 below 2^24 of them).  (b) the cosine's error 2.5e-7 times dist.  (c) the fmaf's one rounding: half an ulp of
#         [64, 128) = 3.815e-6.  A predicted position x + vx is one rounding (c) alone.
#         128 * (2.663e-7 + 2.5e-7) + 3.815e-6 = 6.99e-5 = 18.4 UNIT.
#   vel   VX = fl(fmaf(vr, c, -(vt * s)) + svx), vt = fl(fl(dir_chg * k) * dist).  (a), (b) turn and scale both terms:
#         (|vr| + |vt|) * (2.663e-7 + 2.5e-7) <= 16 * 5.163e-7 = 8.26e-6.  vt's two roundings and the product vt * s: 3 e32 |vt|
#         <= 1.43e-6.  The fmaf (a value below 16): half an ulp of [8, 16) = 4.77e-7; the sum with svx (below 16 too): 4.77e-7.
#         A predicted velocity vx * decay is one rounding, smaller than these.  Together 1.064e-5 = 44.7 UNIT.
#   body  norm_deg_any(fl(body_rel + face)): the one rounding, half an ulp of [256, 512) = 2^-16 = 1 UNIT; the wrap is exact.
DIST_MAX, SPEED_MAX, E32 = 128.0, 8.0, 2.0 ** -24
SINCOS_ERR, ANGLE_ROUND = 2.5e-7, np.radians(2.0 ** -16)
T_ULPS = {'pos': (DIST_MAX * (ANGLE_ROUND + SINCOS_ERR) + 0.5 * float(np.spacing(np.float32(64.0)))) / UNIT['pos'],
          'vel': (2 * SPEED_MAX * (ANGLE_ROUND + SINCOS_ERR) + 3 * E32 * SPEED_MAX + 2 * 0.5 * float(np.spacing(np.float32(8.0))))
          / UNIT['vel'],
          'body': 0.5 * float(np.spacing(np.float32(256.0))) / UNIT['body']}

N_ENT = 22                                               # entry 0 = the ball, entry 1 + j = player row j
X, Y, VX, VY, BODY, PC, VC, BC = range(8)                # words of an entry
COPIED = list(range(16)) + [21, 22, 23]                  # step 3
# see row: continuous words the probes move
SEE_MOVED = [0, 1, 2, 3, 6, 17, 18, 19, 20] + [24 + 8 * r + w for r in range(21) for w in (3, 4, 5, 6, 7)]
BEL_MOVED = [16, 17, 18, 19] + [24 + 8 * j + w for j in range(21) for w in (0, 1, 2, 3)]


def values(**over):
    """the parameters as the layer holds them: belief.DEFAULTS with `over` written over them, every word rounded to fp32 once"""
    v = dict(B.DEFAULTS)
    for k, x in over.items():
        assert k in v, k
        v[k] = x
    return {k: tuple(float(np.float32(a)) for a in x) if isinstance(x, (tuple, list)) else float(np.float32(x)) for k, x in v.items()}


def norm_deg(d):
    with np.errstate(invalid='ignore'):
        d = np.where(np.abs(d) > 360.0, np.fmod(d, 360.0), d)
        d = np.where(d < -180.0, d + 360.0, d)
        return np.where(d > 180.0, d - 360.0, d)


def sincos_deg(th):
    """libm on the remainder of the quadrant: exact at multiples of 90 degrees"""
    with np.errstate(invalid='ignore'):
        q = np.rint(th / 90.0)
        r = np.radians(th - 90.0 * q)
        sr, cr = np.sin(r), np.cos(r)
        k = np.where(np.isfinite(q), np.mod(q, 4.0), 0.0)
    s = np.where(k == 0, sr, np.where(k == 1, cr, np.where(k == 2, -sr, -cr)))
    c = np.where(k == 0, cr, np.where(k == 1, -sr, np.where(k == 2, -cr, sr)))
    return s, c


def atan2_deg(y, x):
    return np.where((x == 0.0) & (y == 0.0), 0.0, np.degrees(np.arctan2(y, x)))


def unpack(rows):
    """belief rows [R, 192] -> entries [R, 22, 8] (the ball's body, vel_count and body_count: 0)"""
    rows = np.asarray(rows)
    E = np.zeros((rows.shape[0], N_ENT, 8), dtype=rows.dtype)
    E[:, 0, :4], E[:, 0, PC] = rows[:, 16:20], rows[:, 20]
    E[:, 1:, :] = rows[:, 24:].reshape(-1, 21, 8)
    return E


# ------------------------------------------------------------------------------------------------ the reference
def update(belief, see, flag, u, P):
    """one update of R agent rows in float64: belief, see [R, 192] (fp32 values), flag [R], u [R] (own index 0..10), P = values()
    -> (rows float64 [R, 192], dict(assign int [R, 21]: the player row each level 1-3 sighting took, -1 dropped, -2 no such
    sighting; ghost bool [R, 22]: the entries step 5 forgot))"""
    b, S = np.asarray(belief, dtype=np.float64), np.asarray(see, dtype=np.float64)
    R = b.shape[0]
    u = np.broadcast_to(np.asarray(u, dtype=np.int64), (R,))
    flag = np.broadcast_to(np.asarray(flag), (R,)).astype(np.int64)
    cm = P['count_max']
    E = unpack(b)
    E[:, 0, VC] = E[:, 0, BC] = cm
    AR = np.arange(R)

    def forget(m):
        E[..., :5][m] = 0.0
        E[..., 5:][m] = cm

    with np.errstate(invalid='ignore', over='ignore'):
        # 1. reset
        forget(np.broadcast_to((flag != 0)[:, None], (R, N_ENT)))
        # 2. predict
        known = E[..., PC] < cm
        decay = np.where(np.arange(N_ENT) == 0, P['ball_decay'], P['player_decay'])[None, :]
        for p, v in ((X, VX), (Y, VY)):
            E[..., p] = np.where(known, E[..., p] + E[..., v], E[..., p])
        for v in (VX, VY):
            E[..., v] = np.where(known, E[..., v] * decay, E[..., v])
        for c in (PC, VC, BC):
            E[..., c] = np.where(E[..., c] + 1.0 < cm, E[..., c] + 1.0, cm)
        forget(E[..., PC] == cm)
        # 4. correct
        sx, sy, svx, svy, face, code = (S[:, i] for i in (0, 1, 2, 3, 6, 7))
        can = (S[:, 8] == 1.0) & (S[:, 15] < CARD_RED)
        rows = S[:, 24:].reshape(R, 21, 8)
        # sightings 0..20 = the player rows, 21 = the ball
        level = np.concatenate([rows[:, :, 0], S[:, 16:17]], axis=1)
        dist = np.concatenate([rows[:, :, 3], S[:, 17:18]], axis=1)
        direc = np.concatenate([rows[:, :, 4], S[:, 18:19]], axis=1)
        dchg = np.concatenate([rows[:, :, 5], S[:, 19:20]], axis=1)
        rchg = np.concatenate([rows[:, :, 6], S[:, 20:21]], axis=1)
        team, unum, brel = rows[:, :, 1], rows[:, :, 2], rows[:, :, 7]
        s, c = sincos_deg(norm_deg(face[:, None] + direc))
        SX, SY = dist * c + sx[:, None], dist * s + sy[:, None]
        vt = (rchg * DEG2RAD_F32) * dist
        SVX = np.where(dist != 0.0, dchg * c - vt * s + svx[:, None], svx[:, None])
        SVY = np.where(dist != 0.0, dchg * s + vt * c + svy[:, None], svy[:, None])
        sbody = norm_deg(brel + face[:, None])
        updated = np.zeros((R, N_ENT), dtype=bool)
        m = can & (level[:, 21] >= 1.0)                                          # the ball
        E[m, 0, X], E[m, 0, Y], E[m, 0, PC] = SX[m, 21], SY[m, 21], 0.0
        updated[m, 0] = True
        m = m & (level[:, 21] == 4.0)
        E[m, 0, VX], E[m, 0, VY] = SVX[m, 21], SVY[m, 21]
        for r in range(21):                                                       # first pass, in row order: the later wins
            un = unum[:, r]
            m = can & (level[:, r] == 4.0) & (un >= 1.0) & (un <= 11.0) & (un == np.rint(un))
            n = np.where(m, un, 1.0).astype(np.int64)
            mate, opp = team[:, r] > 0.0, team[:, r] < 0.0
            j = np.where(mate, np.where(n - 1 < u, n - 1, n - 2), n + 9)
            m = m & ((mate & (n - 1 != u)) | opp)
            i, e = AR[m], 1 + j[m]
            E[i, e, X], E[i, e, Y], E[i, e, VX], E[i, e, VY], E[i, e, BODY] = SX[m, r], SY[m, r], SVX[m, r], SVY[m, r], sbody[m, r]
            E[i, e, PC] = E[i, e, VC] = E[i, e, BC] = 0.0
            updated[i, e] = True
        assign = np.full((R, 21), -2, dtype=np.int64)
        jj = np.arange(21)[None, :]
        for r in range(21):                                                       # second pass, one after the other
            lv = level[:, r]
            m = can & ((lv == 1.0) | (lv == 2.0) | (lv == 3.0))
            if not m.any():
                continue
            t = team[:, r][:, None]
            cand = np.where(t > 0.0, jj < 10, np.where(t < 0.0, jj >= 10, True)) & ~updated[:, 1:] & (E[:, 1:, PC] < cm)
            tol = P['match_rate'] * dist[:, r] + P['match_dist']
            q = (SX[:, r, None] - E[:, 1:, X]) ** 2 + (SY[:, r, None] - E[:, 1:, Y]) ** 2
            ok = cand & (q <= (tol * tol)[:, None]) & m[:, None]
            key = np.where(ok, q, np.inf)
            first = (ok & (key == key.min(axis=1, keepdims=True))).argmax(axis=1)     # the smallest q, ties to the lowest row
            hit = ok.any(axis=1)
            assign[m, r] = np.where(hit, first, -1)[m]
            i, e = AR[hit], 1 + first[hit]
            E[i, e, X], E[i, e, Y], E[i, e, PC] = SX[hit, r], SY[hit, r], 0.0
            updated[i, e] = True
        # 5. ghosts
        wi = np.where(code == 1.0, 0, np.where(code == 3.0, 2, 1))
        cone = 0.5 * np.array(P['view_angle'])[wi] - P['ghost_margin']
        dx, dy = E[..., X] - sx[:, None], E[..., Y] - sy[:, None]
        d = np.hypot(dx, dy)
        rel = np.abs(norm_deg(atan2_deg(dy, dx) - face[:, None]))
        ghost = can[:, None] & ~updated & (E[..., PC] < cm) & (d > 0.0) & (rel <= cone[:, None])
        forget(ghost)
    # 3. copy, and pack
    out = np.zeros((R, B.DIM))
    out[:, COPIED] = S[:, COPIED]
    out[:, 16:20], out[:, 20] = E[:, 0, :4], E[:, 0, PC]
    out[:, 24:] = E[:, 1:, :].reshape(R, 168)
    return out, dict(assign=assign, ghost=ghost)


# ------------------------------------------------------------------------------------------------ the rule
def perturb(a, cols, rs, ulps=PROBE_ULPS):
    """a copy of fp32 rows `a` with the finite words of `cols` moved by 1..ulps fp32 ulps in a random direction"""
    out = np.array(a, dtype=np.float32)
    v = out[:, cols]
    steps = rs.randint(1, ulps + 1, size=v.shape) * rs.choice([-1, 1], size=v.shape)
    steps = np.where(np.isfinite(v), steps, 0)
    for k in range(ulps):
        move = np.abs(steps) > k
        v = np.where(move, np.nextafter(v, np.where(steps > 0, np.float32(np.inf), np.float32(-np.inf))), v)
    out[:, cols] = v
    return out


def _diff(a, b, circ=False):
    """|a - b|; 0 where both are NaN or both the same infinity, inf where only one is NaN"""
    with np.errstate(invalid='ignore'):
        d = np.abs(a - b)
        if circ:
            d = np.minimum(d, np.abs(360.0 - d))
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
    d = np.where(a == b, 0.0, d)
    return np.where(np.isnan(d), np.inf, d)


def in_domain(belief, see, P):
    """the domain T_ULPS is derived for (see its comment), over the finite words"""
    b, S = np.asarray(belief, dtype=np.float64), np.asarray(see, dtype=np.float64)
    ok = lambda v, lim: bool((np.abs(v[np.isfinite(v)]) <= lim).all())          # noqa: E731
    rows = S[:, 24:].reshape(-1, 21, 8)
    dist = np.concatenate([rows[:, :, 3], S[:, 17:18]], axis=1)
    with np.errstate(invalid='ignore', over='ignore'):
        vt = np.concatenate([rows[:, :, 6], S[:, 20:21]], axis=1) * DEG2RAD_F32 * dist
        out = unpack(update(belief, see, 0, 0, P)[0])[..., :2]                  # (u does not move a position, only its row)
    return (ok(dist, DIST_MAX) and ok(out, DIST_MAX) and ok(vt, SPEED_MAX) and ok(rows[:, :, 5], SPEED_MAX) and ok(S[:, 19], SPEED_MAX)
            and ok(b[:, BEL_MOVED], DIST_MAX - 2 * SPEED_MAX) and ok(S[:, 6:7] + rows[:, :, 4], 360.0) and ok(S[:, 6:7] + rows[:, :, 7], 360.0))


def compare(got, belief, see, flag, u, P, T=T_ULPS, seed=0xBE1, probes=K_PROBES):
    """(report, failures) of fp32 rows `got` [R, 192] -- one update of `belief` [R, 192] with `see` [R, 192] -- against float64.
    T = None measures only.  report['worst'][word] = max over well-conditioned rows of (|f32 - f64| - 2 spread) / UNIT, the figure
    held against T; report['raw'][word] = max of |f32 - f64| / UNIT, the deviation itself."""
    belief, see = np.ascontiguousarray(belief, dtype=np.float32), np.ascontiguousarray(see, dtype=np.float32)
    got = np.ascontiguousarray(got, dtype=np.float32)
    R = belief.shape[0]
    assert got.shape == belief.shape == see.shape == (R, B.DIM), (got.shape, belief.shape, see.shape)
    base, disc = update(belief, see, flag, u, P)
    Eb = unpack(base)
    ill = np.zeros(R, dtype=bool)
    spread = np.zeros((R, N_ENT, 5))
    rs = np.random.RandomState(seed)
    for _ in range(probes):
        p, pd = update(perturb(belief, BEL_MOVED, rs), perturb(see, SEE_MOVED, rs), flag, u, P)
        Ep = unpack(p)
        ill |= (pd['assign'] != disc['assign']).any(axis=1) | (pd['ghost'] != disc['ghost']).any(axis=1)
        ill |= (Ep[..., 5:] != Eb[..., 5:]).any(axis=(1, 2))                     # any count (and with pos_count: known or not)
        for w in range(5):
            spread[..., w] = np.maximum(spread[..., w], _diff(Ep[..., w], Eb[..., w], circ=w == BODY))
    well = ~ill
    fails = []
    cm = P['count_max']

    def first(bad, what):
        idx = np.argwhere(bad)
        if len(idx):
            fails.append(f'{what}: {len(idx)} cases; first at {tuple(int(i) for i in idx[0])}')

    first(got[:, COPIED].view(np.int32) != see[:, COPIED].view(np.int32), 'copied self / game words differ from the see row (row, word)')
    Eg = unpack(got.astype(np.float64))
    first((Eg[:, 1:, 5:] != Eb[:, 1:, 5:]) & well[:, None, None], 'a count of a well-conditioned row differs (row, player row, count)')
    first((Eg[:, 0, PC] != Eb[:, 0, PC]) & well, "the ball's pos_count of a well-conditioned row differs (row)")
    unknown = Eb[..., PC] == cm
    bits = unpack(got.view(np.int32))[..., :5]
    first((bits != 0).any(axis=-1) & unknown & well[:, None], 'an unknown entry is not the canonical all-+0 one (row, entry)')
    worst, raw = {}, {}
    for name, words in (('pos', (X, Y)), ('vel', (VX, VY)), ('body', (BODY,))):
        w = list(words)
        err = _diff(Eg[..., w], Eb[..., w], circ=name == 'body')
        with np.errstate(invalid='ignore'):
            excess = (err - 2.0 * spread[..., w]) / UNIT[name]
        excess = np.where(np.isnan(excess), np.where(err == 0.0, -np.inf, np.inf), excess)      # (inf - inf: equal values agree)
        excess = np.where(well[:, None, None], excess, -np.inf)
        worst[name] = float(excess.max()) if excess.size else -np.inf
        raw[name] = float(np.where(well[:, None, None] & np.isfinite(err), err, 0.0).max() / UNIT[name])
        if T is not None and worst[name] > T[name]:
            r, e, k = np.unravel_index(np.argmax(excess), excess.shape)
            fails.append(f'{name}: |f32 - f64| - 2 spread = {worst[name]:.2f} ulps > {T[name]:.2f} at row {r} entry {e} word {w[k]}: '
                         f'f32={float(Eg[r, e, w[k]])!r} f64={float(Eb[r, e, w[k]])!r} spread={float(spread[r, e, w[k]])!r}')
    return dict(n=R, ill=int(ill.sum()), share=float(ill.sum()) / max(R, 1), well=well, worst=worst, raw=raw, f64=base, disc=disc), fails


# ------------------------------------------------------------------------------------------------ random rows
def random_rows(rng, R, P):
    """R random updates inside the domain: (belief, see fp32 [R, 192], flag uint8 [R], slot int [R]).  Each row: an agent somewhere
    on the pitch, 21 players and a ball at true places; a WELL-FORMED see row of them (levels 0..4 at random, dist on a 0.1 grid,
    whole-degree directions, team and unum words as the level allows, seen rows first in ascending direction); a prior belief
    that knows about 60 % of them about a metre from the truth with whole counts in [0, count_max]."""
    f32 = np.float32
    cm = int(P['count_max'])
    slot = rng.integers(0, 22, R)
    u = slot % 11
    S = np.zeros((R, B.DIM), dtype=f32)
    S[:, 0], S[:, 1] = rng.uniform(-52, 52, R), rng.uniform(-34, 34, R)
    S[:, 2:4] = rng.uniform(-1, 1, (R, 2))
    body, neck = rng.uniform(-180, 180, R).astype(f32), rng.uniform(-90, 90, R).astype(f32)
    face = norm_deg((body + neck).astype(np.float64)).astype(f32)
    S[:, 4], S[:, 5], S[:, 6], S[:, 7] = body, neck, face, rng.integers(1, 4, R)
    S[:, 8], S[:, 9] = rng.random(R) < 0.85, rng.integers(0, 4, R)
    S[:, 10:14] = (8000.0, 1.0, 1.0, 130600.0)
    S[:, 14], S[:, 15] = u == 0, rng.choice([0, 0, 0, 0, 0, 0, 1, 2], R)
    S[:, 21], S[:, 22], S[:, 23] = rng.integers(0, 30, R), rng.integers(-1, 2, R), rng.integers(0, 6000, R)
    # the truth: own-frame slots 0..21 and the ball (22)
    tx, ty = rng.uniform(-52, 52, (R, 23)), rng.uniform(-34, 34, (R, 23))
    tvx, tvy = rng.uniform(-1, 1, (R, 23)), rng.uniform(-1, 1, (R, 23))
    tvx[:, 22], tvy[:, 22] = rng.uniform(-2.5, 2.5, R), rng.uniform(-2.5, 2.5, R)
    tbody = rng.uniform(-180, 180, (R, 23))
    sx, sy, svx, svy, fc = (S[:, i].astype(np.float64)[:, None] for i in (0, 1, 2, 3, 6))
    dx, dy = tx - sx, ty - sy
    d = np.hypot(dx, dy)
    rel = np.rint(norm_deg(atan2_deg(dy, dx) - fc))
    dist = np.maximum(np.rint(d * 10.0) / 10.0, 0.1)
    ex, ey = dx / d, dy / d
    rvx, rvy = tvx - svx, tvy - svy
    dist_chg = np.rint((rvx * ex + rvy * ey) * 50.0) / 50.0
    dir_chg = np.rint(np.degrees((rvy * ex - rvx * ey) / d) * 10.0) / 10.0
    dir_chg = np.clip(dir_chg, -0.9 * SPEED_MAX / (DEG2RAD_F32 * dist), 0.9 * SPEED_MAX / (DEG2RAD_F32 * dist))
    brel = np.rint(norm_deg(tbody - fc))
    level = rng.choice([0, 1, 2, 3, 4], (R, 23), p=[0.3, 0.1, 0.2, 0.15, 0.25])
    level[:, 22] = rng.choice([0, 1, 4], R, p=[0.3, 0.2, 0.5])
    me = (slot % 11)                                      # the agent's own own-frame slot
    level[np.arange(R), me] = 0
    k = np.arange(22)[None, :]
    lv = level[:, :22]
    words = np.stack([lv, np.where(lv >= 3, np.where(k < 11, 1.0, -1.0), 0.0), np.where(lv == 4, k % 11 + 1, 0), dist[:, :22], rel[:, :22],
                      np.where(lv == 4, dist_chg[:, :22], 0.0), np.where(lv == 4, dir_chg[:, :22], 0.0), np.where(lv == 4, brel[:, :22], 0.0)],
                     axis=-1)
    words = np.where((lv >= 1)[..., None], words, 0.0)
    order = np.argsort(np.where(lv >= 1, rel[:, :22], np.inf), axis=1, kind='stable')
    words = np.take_along_axis(words, order[..., None], axis=1)[:, :21]
    S[:, 24:] = words.reshape(R, 168)
    bl = level[:, 22]
    S[:, 16], S[:, 17], S[:, 18] = bl, np.where(bl >= 1, dist[:, 22], 0.0), np.where(bl >= 1, rel[:, 22], 0.0)
    S[:, 19], S[:, 20] = np.where(bl == 4, dist_chg[:, 22], 0.0), np.where(bl == 4, dir_chg[:, 22], 0.0)
    # the prior belief: what the agent remembers of the cycle before
    bel = B.unknown(R, 1, f32(cm))[:, 0]
    E = np.zeros((R, N_ENT, 8))
    obj = np.zeros((R, N_ENT), dtype=np.int64)            # the own-frame slot of each entry
    obj[:, 0] = 22
    for j in range(21):
        obj[:, 1 + j] = np.where(j < 10, np.where(j < u, j, j + 1), j + 1)
    px, py = np.take_along_axis(tx - tvx, obj, 1), np.take_along_axis(ty - tvy, obj, 1)
    E[..., X], E[..., Y] = px + rng.normal(0, 1.0, px.shape), py + rng.normal(0, 1.0, px.shape)
    E[..., VX], E[..., VY] = np.take_along_axis(tvx, obj, 1) + rng.normal(0, 0.1, px.shape), np.take_along_axis(tvy, obj, 1) + rng.normal(0, 0.1, px.shape)
    E[..., BODY] = rng.uniform(-180, 180, px.shape)
    hi = max(min(cm, 12), 1)
    E[..., PC] = rng.integers(0, hi, px.shape)
    E[..., VC] = np.minimum(E[..., PC] + rng.integers(0, hi, px.shape), cm)
    E[..., BC] = np.minimum(E[..., PC] + rng.integers(0, hi, px.shape), cm)
    old = rng.random(px.shape) < 0.03                     # about to be forgotten for age
    E[..., PC] = np.where(old, cm - 1, E[..., PC])
    E[..., VC], E[..., BC] = np.maximum(E[..., VC], E[..., PC]), np.maximum(E[..., BC], E[..., PC])
    unknown = rng.random(px.shape) < 0.4
    E[unknown, :5], E[unknown, 5:] = 0.0, cm
    bel[:, 16:20], bel[:, 20] = E[:, 0, :4], E[:, 0, PC]
    bel[:, 24:] = E[:, 1:].reshape(R, 168)
    flag = (rng.random(R) < 0.1).astype(np.uint8)
    return bel, S, flag, slot


def restatement(ref, over, belief, see, flag, slot):
    """one update of R independent rows through tests/belief_ref.c (ref = belief.build(..)): each row a match of its own with the
    one-slot mask of its agent; parameters belief.DEFAULTS with `over` written over them"""
    belief, see = np.ascontiguousarray(belief, dtype=np.float32), np.ascontiguousarray(see, dtype=np.float32)
    flag, slot = np.asarray(flag, dtype=np.uint8), np.asarray(slot)
    out = np.zeros_like(belief)
    prm = B.params(**over)
    for m in np.unique(slot):
        sel = slot == m
        out[sel] = B.step(ref, prm, see[sel][:, None], belief[sel][:, None], flag[sel], mask=1 << int(m))[:, 0]
    return out
