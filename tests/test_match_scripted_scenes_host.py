"""The scene table of tests/scripted_scenes.py on the CPU, three ways: through the host restatement (tests/scripted_policy_ref.c),
through the unprobed float64 rule table (tests/scripted_f64.py), and by the float64 rule with its probes.  Every hand-written answer
must come out of all three.  And the table's coverage of the restatement, measured with gcov as tests/match_coverage.py measures
tests/match_scenes.py: every line and every branch direction of one_match and turn_or_dash, minus ALLOW."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import scripted_f64 as F
import scripted_policy as SP
import scripted_scenes as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# branch directions of the rule function that no state can take: (function, source text of the line, index in gcov's list)
ALLOW = ()
COVERED = ('one_match', 'turn_or_dash')


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return SP.build(tmp_path_factory.mktemp('scripted_scenes'))


@pytest.mark.parametrize('hetero', [False, True])
def test_scene_table_three_ways(ref, hetero):
    cfg = SS.scene_config(hetero)
    prm = SP.params(cfg)
    table = SS.scenes(cfg)
    state, cmd, rule, angles = SS.batch(table)
    assert len({sc.name for sc in table}) == len(table)
    # 1. the restatement: commands and the hand-written angles
    got = SP.actions(ref, state, prm)
    fails = SS.check(table, cmd, rule, angles, got[..., 0], got_ang=F.angle_of(got))
    assert not fails, '\n'.join(['restatement:'] + fails)
    # 2. unprobed float64: commands, rule numbers, angles
    ref64 = F.decide(state, prm)
    fails = SS.check(table, cmd, rule, angles, ref64['cmd'], ref64['rule'], ref64['ang'])
    assert not fails, '\n'.join(['float64:'] + fails)
    # 3. the rule: the restatement against probed float64, and the answers on the rows it holds
    rep, fails = F.compare(state, prm, got)
    print(f'{len(table)} scenes ({"hetero" if hetero else "default"}): ill-conditioned {rep["ill"]} / {rep["n"]} rows = '
          f'{100 * rep["share"]:.2f} %, worst {rep["worst"]}')
    assert not fails, fails
    assert rep['share'] <= F.EDGE_ILL_CAP
    fails = SS.check(table, cmd, rule, angles, got[..., 0], rep['f64']['rule'], F.angle_of(got), rows=rep['well'])
    assert not fails, '\n'.join(['by the rule:'] + fails)


def test_right_versions_are_the_swap(ref):
    """a swapped scene answers with the swapped commands of its left version (the restatement, exact words but the angles)"""
    cfg = SS.scene_config(True)
    table = SS.scenes(cfg)
    state, *_ = SS.batch(table)
    got = SP.actions(ref, state, SP.params(cfg))
    pairs = [(e - 1, e) for e, sc in enumerate(table) if sc.name.endswith(' (right)')]
    assert len(pairs) > 50
    for a, b in pairs:
        assert np.array_equal(got[a, :, 0], got[b, np.r_[11:22, 0:11], 0]), table[a].name


_RUN = """
import sys
sys.path[:0] = [{amd!r}, {tests!r}]
import ctypes as C
import scripted_policy as SP, scripted_scenes as SS
L = C.CDLL({so!r})
L.s2dsp_actions.restype = None
L.s2dsp_actions.argtypes = [C.c_int64] + [C.c_void_p] * 15
for hetero in (False, True):
    cfg = SS.scene_config(hetero)
    state = SS.batch(SS.scenes(cfg))[0]
    SP.actions(L, state, SP.params(cfg))
"""


@pytest.mark.skipif(shutil.which('gcc') is None or shutil.which('gcov') is None, reason='needs gcc and gcov')
def test_scene_table_covers_the_restatement(tmp_path):
    d = str(tmp_path)
    obj, so = os.path.join(d, 'scripted_policy_ref.o'), os.path.join(d, 'libscripted_policy_cov.so')
    for cmd in (['gcc', '--coverage', '-O0', '-ffp-contract=off', '-fPIC', '-c', '-o', obj, SP.SRC],
                ['gcc', '--coverage', '-shared', '-o', so, obj]):
        subprocess.run(cmd, check=True, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    script = _RUN.format(amd=os.path.join(ROOT, 'gym-soccer-2d-env_amd'), tests=os.path.join(ROOT, 'tests'), so=so)
    subprocess.run([sys.executable, '-c', script], check=True, cwd=d)          # the counters are written when it exits
    subprocess.run(['gcov', '--json-format', '-b', 'scripted_policy_ref.o'], check=True, cwd=d, stdout=subprocess.PIPE,
                   stderr=subprocess.STDOUT)
    (name,) = [f for f in os.listdir(d) if f.endswith('.gcov.json.gz')]
    with gzip.open(os.path.join(d, name), 'rt') as fh:
        doc = json.load(fh)
    (rec,) = [f for f in doc['files'] if os.path.basename(f['file']) == os.path.basename(SP.SRC)]
    with open(SP.SRC) as fh:
        src = fh.read().split('\n')
    lines = [ln for ln in rec['lines'] if ln.get('function_name') in COVERED]
    assert {ln['function_name'] for ln in lines} == set(COVERED)
    missed_lines = [ln['line_number'] for ln in lines if ln['count'] == 0]
    missed, total = [], 0
    for ln in lines:
        text = src[ln['line_number'] - 1]
        for k, b in enumerate(ln['branches']):
            total += 1
            if b['count'] == 0 and not any(fn == ln['function_name'] and t in text and i == k for fn, t, i in ALLOW):
                missed.append(f'{ln["line_number"]}#{k}: {text.strip()[:120]}')
    print(f'lines {len(lines) - len(missed_lines)} / {len(lines)}, branch directions {total - len(missed)} / {total} '
          f'(allowed: {len(ALLOW)})')
    assert not missed_lines, missed_lines
    assert not missed, '\n'.join(missed)
