"""The rule-scene table (tests/match_scenes.py) on the fp32 match oracle: every scene reaches the rule it is named after, and the table
as a whole reaches every line and every branch direction of the oracle's step and reset path -- measured with gcov on an instrumented
build -- but the few directions of match_scenes.ALLOW, each with its reason.  What the table reaches on the oracle is what
tests/test_gpu_match_scenes.py compares on the kernel."""
import os
import subprocess
import sys

import pytest

import match_coverage as MC
import match_scenes as MS

ALLOW_SHARE = 0.03                 # of the path's branch directions, at the most


@pytest.mark.parametrize('sc', MS.SCENES, ids=[s.name for s in MS.SCENES])
def test_scene_reaches_its_rule(sc):
    assert sc.n <= 64 and sc.T <= 400
    tr = MS.run_on_oracle(sc)
    assert tr['mode'].shape == (sc.T, sc.n)
    assert sc.witness(tr), f'{sc.name}: the witness does not hold on the oracle'


def test_scene_names_are_unique_and_the_stock_kernel_is_driven():
    names = [s.name for s in MS.SCENES]
    assert len(set(names)) == len(names)
    assert sum(MS.stock_accepts(s) for s in MS.SCENES) >= len(names) // 2


def _allowed(missed_branches, missed_lines):
    """split gcov's misses into those ALLOW names (by the source text of their line) and the rest"""
    src = MC.source_lines()
    texts = [t for t, _why in MS.ALLOW]
    for t, why in MS.ALLOW:
        assert sum(t in ln for ln in src) == 1, f'ALLOW entry matches no line or several: {t!r}'
        assert why.strip().endswith('.') and len(why) > 30, f'ALLOW entry without a reason: {t!r}'
    ok = lambda no: any(t in src[no - 1] for t in texts)
    return ([b for b in missed_branches if ok(b[0])], [b for b in missed_branches if not ok(b[0])],
            [no for no in missed_lines if not ok(no)])


@pytest.mark.skipif(not MC.have_tools(), reason='gcc or gcov is not on PATH')
def test_table_covers_the_step_and_reset_path(tmp_path):
    lib = MC.build(str(tmp_path))
    # a fresh child: the counters are written when it exits
    env = dict(os.environ, OMP_NUM_THREADS='2')
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(MC.__file__)), 'match_coverage.py'), 'run', str(tmp_path)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert os.path.exists(lib) and os.path.exists(os.path.join(str(tmp_path), 's2d_match_oracle.gcda')), 'the child left no counters'
    s = MC.summary(MC.report(str(tmp_path)))
    allowed, missed, missed_lines = _allowed(s['missed_branches'], s['missed_lines'])
    src = MC.source_lines()
    print('step and reset path: lines %d / %d, branch directions %d / %d, %d allowed' % (s['lines'] + s['branches'] + (len(allowed),)))
    assert s['lines'][1] > 500 and s['branches'][1] > 700, 'gcov saw too little of the source: the path filter is broken'
    assert not missed_lines, 'lines no scene reaches:\n' + '\n'.join(f'{no}: {src[no - 1].strip()}' for no in missed_lines)
    assert not missed, 'branch directions no scene reaches:\n' + '\n'.join(f'{no}#{k}: {src[no - 1].strip()}' for no, k in missed)
    assert len(allowed) <= ALLOW_SHARE * s['branches'][1], (len(allowed), s['branches'][1])
    # an allow-list entry that a scene does reach is stale: take it out
    hit = {no for no, _k in allowed}
    stale = [t for t, _why in MS.ALLOW if not any(t in src[no - 1] for no in hit)]
    assert not stale, f'ALLOW entries whose line is fully covered: {stale}'
