"""The belief kernels behind the raw C ABI (s2d_match_belief_scan, s2d_match_belief_reset; include/s2d_match.h, "Belief") at their
edges: the constructed scenes of tests/belief_scenes.py (known answers), every agent count around the block of 8 half-waves, every
kind of slot mask, T = 1, 2, 3 and 33 with and without the record and the reset flags, on a stream of its own, and every refusal.
Every device array is followed by sentinel words (as tests/test_gpu_learn.DevLearner's), which are checked after every call; the
inputs are checked to be unchanged.  Bit for bit against the host restatement (tests/belief_ref.c); NaN matches NaN."""
import ctypes as C

import numpy as np
import pytest

import belief as B
import belief_f64 as F
import belief_scenes as SC
from soccer2d_amd import _capi, _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
DEV = 'cuda:0'
PAD, S_F, S_B = 64, -7777.0, 0xA5
ALL, LEFT, RIGHT = 0x3FFFFF, 0x7FF, 0x3FF800
OTHER = dict(ball_decay=0.9, player_decay=0.5, view_angle=(50.0, 100.0, 170.0), match_dist=2.0, match_rate=0.05, ghost_margin=3.0,
             count_max=6.0)
AGENTS = (1, 2, 7, 8, 9, 15, 16, 17, 8 * 64 + 3)           # n * k around the 8 agents of a block, and many blocks
# (n_matches, mask): every agent count with a one-slot mask; the masks of 11 and 22 slots at counts beside and on a multiple of 8
SHAPES = [(a, 1 << ((5 * i + 3) % 22)) for i, a in enumerate(AGENTS)] + [(1, LEFT), (3, RIGHT), (8, LEFT), (16, RIGHT), (1, ALL), (3, ALL), (4, ALL)]
SHAPE_IDS = [f'{n}x{bin(m).count("1")}' for n, m in SHAPES]
_rs = np.random.RandomState(22)
RANDOM_MASKS = [int(sum(1 << int(b) for b in _rs.choice(22, size=k, replace=False))) for k in (2, 7, 16)]
MASKS = [1 << s for s in range(22)] + [LEFT, RIGHT] + RANDOM_MASKS
STEPS = [(T, rec, rst) for T in (1, 2, 3, 33) for rec in (True, False) for rst in (True, False)]


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return B.build(tmp_path_factory.mktemp('belief_ref'))


@pytest.fixture(scope='module')
def lib():
    return M.bind(_capi.load_library())


def same(got, want, what):
    """tests/test_gpu_learn.same's rule: bit for bit, the sign of zero included; NaN matches NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got.view(np.int32) != want.view(np.int32)))
    if bad.any():
        idx = np.argwhere(bad)
        i = tuple(idx[0])
        raise AssertionError(f'{what}: {len(idx)} of {got.size} words differ; first at {i}: gpu={got[i]!r} want={want[i]!r}')


class Guarded:
    """a device array with PAD sentinel words behind it"""

    def __init__(self, a=None, words=0, dtype=torch.float32):
        self.fill = S_F if dtype == torch.float32 else S_B
        self.n = int(a.size) if a is not None else words
        self.t = torch.full((self.n + PAD,), self.fill, dtype=dtype, device=DEV)
        self.given = None
        if a is not None:
            self.given = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV)
            self.t[:self.n] = self.given

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.t[self.n:] == self.fill).all())

    def unchanged(self):
        """bit for bit what was given (or, for an output never written, still all sentinels)"""
        if self.given is None:
            return bool((self.t == self.fill).all())
        a, b = self.t[:self.n], self.given
        return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b))

    def numpy(self, shape):
        return self.t[:self.n].cpu().numpy().reshape(shape)


def launch(lib, over, see, belief, reset=None, mask=ALL, record=True, stream=None):
    """one s2d_match_belief_scan on guarded device copies: see [T, n, k, 192], belief [n, k, 192], reset uint8 [T, n] or None ->
    (the belief afterwards, the record or None).  Checks the return code, every guard, and that see and reset are unchanged."""
    T, n, k, d = see.shape
    assert d == 192 and k == B.popcount(mask) and belief.shape == (n, k, 192) and (reset is None or reset.shape == (T, n))
    prm = M.belief_params(lib, **over)
    s, b = Guarded(see.astype(np.float32)), Guarded(belief.astype(np.float32))
    r = Guarded(reset.astype(np.uint8), dtype=torch.uint8) if reset is not None else None
    o = Guarded(words=see.size) if record else None
    torch.cuda.synchronize()
    rc = lib.s2d_match_belief_scan(C.byref(prm), s.ptr, r.ptr if r else None, b.ptr, o.ptr if o else None, T, n, mask,
                                   stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    _capi.check(lib, rc, 's2d_match_belief_scan')
    for g, name in ((s, 'see_dev'), (b, 'belief_dev'), (r, 'reset_dev'), (o, 'out_dev')):
        assert g is None or g.guards_intact(), f'wrote past {name}'
    assert s.unchanged() and (r is None or r.unchanged()), 'an input was written'
    return b.numpy(belief.shape), o.numpy(see.shape) if o else None


def random_record(seed, T, n, k, over):
    """random well-formed see rows [T, n, k, 192], a random prior belief [n, k, 192] and reset flags [T, n]"""
    P = F.values(**over)
    bel, see, flag, _slot = F.random_rows(np.random.default_rng(seed), T * n * k, P)
    return see.reshape(T, n, k, 192), bel[:n * k].reshape(n, k, 192), flag[:T * n].reshape(T, n)


def test_cases_cover_every_axis_value():
    """so that a later edit cannot quietly drop an axis value"""
    counts = {n * B.popcount(m) for n, m in SHAPES}
    assert counts >= set(AGENTS) and {B.popcount(m) for n, m in SHAPES} == {1, 11, 22}
    assert any(c % 8 == 0 for c in counts) and any(B.popcount(m) > 1 and (n * B.popcount(m)) % 8 == 0 for n, m in SHAPES)
    assert {m for m in MASKS if B.popcount(m) == 1} == {1 << s for s in range(22)} and LEFT in MASKS and RIGHT in MASKS
    assert len(RANDOM_MASKS) == 3 and all(B.popcount(m) not in (1, 11, 22) for m in RANDOM_MASKS)
    assert {T for T, _, _ in STEPS} == {1, 2, 3, 33} and {(rec, rst) for _, rec, rst in STEPS} == {(a, b) for a in (True, False) for b in (True, False)}
    T = SC.table()
    assert {s.bullet for s in T} == set(SC.BULLETS) and {s.prm for s in T} == set(SC.PARAMS)


@pytest.mark.parametrize('prm', list(SC.PARAMS))
def test_scenes(lib, ref, prm):
    """the scene table, one launch per parameter set: a scene for slot s sits in row s of a 22-row match"""
    scenes = [s for s in SC.table() if s.prm == prm]
    over = SC.PARAMS[prm]
    bel, see, reset, where = SC.pack(scenes)
    got, rec = launch(lib, over, see[None], bel, reset[None], ALL)
    same(got, B.step(ref, B.params(**over), see, bel, reset, ALL), f'scenes [{prm}] against the restatement')
    same(rec[0], got, 'the record')
    wrong = []
    for s, (m, row) in zip(scenes, where):
        want = s.answer()
        d = SC.same_row(got[m, row], want)
        if len(d):
            wrong.append(f'{s.name}: word {d[0]}: {got[m, row, d[0]]!r}, the answer is {want[d[0]]!r} ({len(d)} words differ)')
    assert not wrong, '\n'.join(wrong)
    # the free rows: a blank see row over an unknown belief stays unknown
    used = np.zeros(got.shape[:2], dtype=bool)
    for m, row in where:
        used[m, row] = True
    same(got[~used], B.unknown(1, int((~used).sum()), np.float32(scenes[0].cm))[0], 'free rows')


@pytest.mark.parametrize('n, mask', SHAPES, ids=SHAPE_IDS)
def test_agent_counts(lib, ref, n, mask):
    k = B.popcount(mask)
    see, bel, flag = random_record(n * 31 + k, 2, n, k, {})
    got, rec = launch(lib, {}, see, bel, flag, mask)
    hfin, hrec = B.scan(ref, B.params(), see, bel, flag, mask)
    same(rec, hrec, f'{n} x {k}: record')
    same(got, hfin, f'{n} x {k}: final')


@pytest.mark.parametrize('n, mask', SHAPES, ids=SHAPE_IDS)
def test_reset(lib, ref, n, mask):
    """s2d_match_belief_reset with and without a match mask, guards behind both arrays"""
    k = B.popcount(mask)
    rng = np.random.default_rng(n + k)
    before = rng.normal(size=(n, k, 192)).astype(np.float32)
    for m in (None, (rng.random(n) < 0.5).astype(np.uint8), np.zeros(n, dtype=np.uint8), np.full(n, 255, dtype=np.uint8)):
        b = Guarded(before)
        g = Guarded(m, dtype=torch.uint8) if m is not None else None
        torch.cuda.synchronize()
        rc = lib.s2d_match_belief_reset(b.ptr, n, mask, g.ptr if g else None, None)
        torch.cuda.synchronize()
        _capi.check(lib, rc, 's2d_match_belief_reset')
        assert b.guards_intact() and (g is None or (g.guards_intact() and g.unchanged()))
        same(b.numpy(before.shape), B.reset(ref, before, m), f'reset {n} x {k}')


def test_masks(lib, ref):
    """every one-slot mask, left, right and three random masks: the restatement's rows, and the matching rows of an `all` launch
    on the same see rows (a row depends on its own see row and u only)"""
    n, T = 5, 2
    see, bel, flag = random_record(77, T, n, 22, OTHER)
    full, full_rec = launch(lib, OTHER, see, bel, flag, ALL)
    same(full_rec, B.scan(ref, B.params(**OTHER), see, bel, flag, ALL)[1], 'all')
    for mask in MASKS:
        rows = [s for s in range(22) if (mask >> s) & 1]
        s, b = np.ascontiguousarray(see[:, :, rows]), np.ascontiguousarray(bel[:, rows])
        got, rec = launch(lib, OTHER, s, b, flag, mask)
        same(rec, B.scan(ref, B.params(**OTHER), s, b, flag, mask)[1], f'mask {mask:#x}')
        same(rec, full_rec[:, :, rows], f'mask {mask:#x} against the rows of the all launch')
        same(got, full[:, rows], f'mask {mask:#x}: final')


@pytest.mark.parametrize('T, record, with_reset', STEPS)
def test_steps_and_arguments(lib, ref, T, record, with_reset):
    """the scan equals T single steps (the kernel prefetches row t + 1: T = 1, 2, 3 are its edges), on a stream of its own"""
    n, mask = 3, RANDOM_MASKS[1]
    k = B.popcount(mask)
    see, bel, _ = random_record(1000 + T, T, n, k, {})
    flag = ((np.arange(T)[:, None] + np.arange(n)[None, :]) % 3 == 0).astype(np.uint8)      # set and clear in every row, T = 1 too
    reset = flag if with_reset else None
    stream = torch.cuda.Stream()
    got, rec = launch(lib, {}, see, bel, reset, mask, record, stream)
    hfin, hrec = B.scan(ref, B.params(), see, bel, reset, mask)
    same(got, hfin, 'final')
    if record:
        same(rec, hrec, 'record')
        same(rec[-1], got, 'the last row of the record is the state')
    b = bel
    for t in range(T):
        b, _ = launch(lib, {}, see[t:t + 1], b, None if reset is None else reset[t:t + 1], mask, False)
        if record:
            same(b, rec[t], f'step {t}')
    same(b, got, 'T single steps')


def test_refusals(lib):
    """every refusal the header lists, for both entry points: S2D_EINVAL with its text, before anything is written"""
    n, T, mask = 4, 3, ALL
    state = n * 22 * 192
    prm = M.belief_params(lib)
    see, bel, out = Guarded(words=2 * T * state), Guarded(words=2 * state), Guarded(words=2 * T * state)   # room for the shifted pointers
    rst = Guarded(words=T * n, dtype=torch.uint8)
    P = C.byref(prm)

    def untouched():
        torch.cuda.synchronize()
        assert see.unchanged() and bel.unchanged() and out.unchanged() and rst.unchanged()

    def scan(word, prm=P, s=see.ptr, r=rst.ptr, b=bel.ptr, o=out.ptr, T=T, n=n, mask=mask):
        assert lib.s2d_match_belief_scan(prm, s, r, b, o, T, n, mask, None) == _capi.S2D_EINVAL, word
        assert word in lib.s2d_last_error().decode(), (word, lib.s2d_last_error())
        untouched()

    scan('non-NULL', prm=None); scan('non-NULL', s=None); scan('non-NULL', b=None)
    scan('slot_mask', mask=0); scan('slot_mask', mask=1 << 22); scan('slot_mask', mask=0xFFFFFFFF)
    scan('n_matches', n=0); scan('n_matches', n=-1); scan('n_matches', n=(1 << 24) + 1)
    scan('n_steps', T=0); scan('n_steps', T=-3)
    for off in (4, 8, 12):                                 # a pointer off by one, two or three words
        scan('aligned', s=see.ptr + off); scan('aligned', b=bel.ptr + off); scan('aligned', o=out.ptr + off)
    byts = 4 * state
    scan('overlaps', o=bel.ptr); scan('overlaps', o=see.ptr)
    scan('overlaps', o=bel.ptr + byts - 16); scan('overlaps', o=see.ptr + T * byts - 16)       # the last 16 bytes of either
    scan('overlaps', b=out.ptr + T * byts - 16)             # the state begins inside the record's last row
    scan('overlaps', b=see.ptr + 16, o=None); scan('overlaps', b=see.ptr + T * byts - 16, o=None); scan('overlaps', s=bel.ptr + byts - 16)
    bad = [('ball_decay', 0.0), ('ball_decay', 1.5), ('player_decay', -0.1), ('player_decay', float('nan')), ('match_dist', -1.0),
           ('match_rate', -0.5), ('match_rate', float('inf')), ('ghost_margin', -1.0), ('count_max', 0.0), ('count_max', 2.5),
           ('count_max', 2.0 ** 24 + 2), ('view_angle', 0.0), ('view_angle', 400.0), ('view_angle', float('nan'))]
    texts = {'ball_decay': 'decay', 'player_decay': 'decay', 'match_dist': 'match_dist', 'match_rate': 'match_dist',
             'ghost_margin': 'match_dist', 'count_max': 'count_max', 'view_angle': 'view_angle'}
    for name, v in bad:
        for i in range(3 if name == 'view_angle' else 1):
            q = M.S2DBeliefParams.from_buffer_copy(prm)
            if name == 'view_angle':
                q.view_angle[i] = v
            else:
                setattr(q, name, v)
            scan('finite' if v != v or abs(v) == float('inf') else texts[name], prm=C.byref(q))
            assert lib.s2d_match_belief_validate(C.byref(q)) == _capi.S2D_EINVAL

    def reset(word, b=bel.ptr, n=n, mask=mask):
        assert lib.s2d_match_belief_reset(b, n, mask, rst.ptr, None) == _capi.S2D_EINVAL, word
        assert word in lib.s2d_last_error().decode(), (word, lib.s2d_last_error())
        untouched()

    reset('NULL', b=None); reset('aligned', b=bel.ptr + 4); reset('aligned', b=bel.ptr + 8)
    reset('n_matches', n=0); reset('n_matches', n=(1 << 24) + 1); reset('slot_mask', mask=0); reset('slot_mask', mask=1 << 22)
    assert see.guards_intact() and bel.guards_intact() and out.guards_intact() and rst.guards_intact()
