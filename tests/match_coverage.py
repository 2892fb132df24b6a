"""gcov bookkeeping for the fp32 match oracle (oracle/s2d_match_oracle.c).  TEST INFRASTRUCTURE.

`build(dir)` makes the `coverage` target of oracle/Makefile into `dir`, `report(dir)` runs `gcov --json-format -b` there and
`summary(...)` counts the lines and branch directions of the STEP AND RESET PATH that were reached: every function of
s2d_match_oracle.c except the accessors a test reads and writes the state with, and the argument guard of s2dmo_create.
A branch direction is one entry of gcov's per-line `branches` list (-O0: one pair per condition of the source).

By hand:  python tests/match_coverage.py build DIR | report DIR [--missed] | run DIR (the scene table against DIR's library)
"""
import gzip
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, 'oracle')
SOURCE = 's2d_match_oracle.c'
LIB = 'libs2d_match_oracle_f32.so'

# not on the step and reset path: what a test reads and writes the state with
ACCESSORS = frozenset(('s2dmo_get', 's2dmo_set_obj', 's2dmo_set_card', 's2dmo_set_touch', 's2dmo_set_game', 's2dmo_stats',
                       's2dmo_relative', 's2dmo_load', 's2dmo_set_env_ids', 's2dmo_events'))
GUARD_LINES = {'s2dmo_create': ('if (!cfg || n <= 0) return NULL;',)}      # argument guards: the source text of the excluded lines


def have_tools():
    return shutil.which('gcc') is not None and shutil.which('gcov') is not None


def build(out_dir):
    """the instrumented library in out_dir (with its .gcno beside it); returns its path"""
    out_dir = os.path.abspath(out_dir)
    subprocess.run(['make', '-B', '-C', ORACLE_DIR, 'coverage', 'CC=gcc', f'COV={out_dir}'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return os.path.join(out_dir, LIB)


def report(out_dir):
    """gcov's JSON record of SOURCE from the counters in out_dir"""
    out_dir = os.path.abspath(out_dir)
    for f in os.listdir(out_dir):
        if f.endswith('.gcov.json.gz'):
            os.remove(os.path.join(out_dir, f))
    subprocess.run(['gcov', '--json-format', '-b', 's2d_match_oracle.o'], cwd=out_dir, check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    (name,) = [f for f in os.listdir(out_dir) if f.endswith('.gcov.json.gz')]
    with gzip.open(os.path.join(out_dir, name), 'rt') as fh:
        doc = json.load(fh)
    (rec,) = [f for f in doc['files'] if os.path.basename(f['file']) == SOURCE]
    return rec


def source_lines():
    with open(os.path.join(ORACLE_DIR, SOURCE)) as fh:
        return fh.read().split('\n')


def path_lines(rec):
    """gcov's line records of the step and reset path: [(line number, function, count, [branch counts])]"""
    src = source_lines()
    out = []
    for ln in rec['lines']:
        fn = ln.get('function_name', '')
        base = fn.split('.')[0]                            # s2dmo_step._omp_fn.0: the body of its OpenMP region
        if base in ACCESSORS:
            continue
        text = src[ln['line_number'] - 1]
        if any(g in text for g in GUARD_LINES.get(base, ())):
            continue
        out.append((ln['line_number'], fn, ln['count'], [b['count'] for b in ln['branches']]))
    return out


def summary(rec):
    """{'lines': (reached, all), 'branches': (reached, all), 'missed_lines': [line], 'missed_branches': [(line, index)]}"""
    lines = path_lines(rec)
    # a source line may be recorded once per function it belongs to (the OpenMP region): a line counts once, its branches per record
    by_line = {}
    for no, _fn, cnt, _br in lines:
        by_line[no] = max(by_line.get(no, 0), cnt)
    missed_lines = sorted(no for no, c in by_line.items() if c == 0)
    allb, missed = 0, []
    seen = {}
    for no, _fn, _cnt, br in lines:
        for b in br:
            k = seen.get(no, 0)
            seen[no] = k + 1
            allb += 1
            if b == 0:
                missed.append((no, k))
    return dict(lines=(len(by_line) - len(missed_lines), len(by_line)), branches=(allb - len(missed), allb),
                missed_lines=missed_lines, missed_branches=missed)


def run_table(lib_path, names=None):
    """every scene of the table (or those named) on the library at lib_path; this process's f32 match oracle from then on"""
    sys.path[:0] = [p for p in (os.path.join(ROOT, 'gym-soccer-2d-env_amd'), os.path.join(ROOT, 'tests')) if p not in sys.path]
    import match_oracle as MO
    import match_scenes as MS
    MO.use_library(lib_path)
    for sc in MS.SCENES:
        if names is None or sc.name in names:
            MS.run_on_oracle(sc)


def format_missed(rec):
    src = source_lines()
    s = summary(rec)
    out = ['lines %d / %d, branch directions %d / %d' % (s['lines'] + s['branches'])]
    for no in s['missed_lines']:
        out.append(f'line   {no}: {src[no - 1].strip()[:150]}')
    for no, k in s['missed_branches']:
        out.append(f'branch {no}#{k}: {src[no - 1].strip()[:150]}')
    return '\n'.join(out)


if __name__ == '__main__':
    cmd, d = sys.argv[1], sys.argv[2]
    if cmd == 'build':
        print(build(d))
    elif cmd == 'run':
        skip = [a[len('--without='):] for a in sys.argv[3:] if a.startswith('--without=')]
        if skip:
            sys.path[:0] = [os.path.join(ROOT, 'gym-soccer-2d-env_amd'), os.path.join(ROOT, 'tests')]
            import match_scenes as MS
            run_table(os.path.join(os.path.abspath(d), LIB), [s.name for s in MS.SCENES if s.name not in skip])
        else:
            run_table(os.path.join(os.path.abspath(d), LIB))
    elif cmd == 'report':
        rec = report(d)
        if '--json' in sys.argv:
            json.dump(rec, open(sys.argv[sys.argv.index('--json') + 1], 'w'))
        print(format_missed(rec) if '--missed' in sys.argv else 'lines %d / %d, branch directions %d / %d' %
              (summary(rec)['lines'] + summary(rec)['branches']))
