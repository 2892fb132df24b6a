"""Compare the device code of two source trees kernel by kernel (the method of profiles/r05/qnet_actor_isa.txt).

Every unit of gym-soccer-2d-env_amd/csrc (SRCS of the new tree's Makefile) is compiled in both trees with the flags of the Makefile plus --cuda-device-only,
llvm-objdump -d splits the code object into kernel symbols, and each kernel's instructions are compared one by one:
comments, <symbol> targets, s_nop 0 and end-of-function padding stripped, PC-relative literals masked.  No GPU needed.

    python profiles/experiments/isa_compare.py OLD_TREE NEW_TREE [--rename OLD_SYM=NEW_SYM ...] [--new-template-arg TEXT ...]

--new-template-arg 'QNetDims, ': a kernel template of the new tree has gained the template argument TEXT; an old symbol is compared
with the new symbol whose demangled name is the old one's once the first TEXT is taken out.  A unit that only the new tree has is listed as new.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
HIPCC = os.path.join(ROCM, 'bin', 'hipcc')
OBJDUMP = os.path.join(ROCM, 'llvm', 'bin', 'llvm-objdump')
FLAGS = ['-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-fPIC', '-fvisibility=hidden', '--cuda-device-only',
         '--no-gpu-bundle-output']


def units(tree):
    """the translation units of the library: SRCS of the tree's csrc/Makefile"""
    with open(os.path.join(tree, 'gym-soccer-2d-env_amd', 'csrc', 'Makefile')) as f:
        m = re.search(r'^SRCS\s*:?=\s*((?:.*\\\n)*.*)$', f.read(), re.M)
    if not m:
        sys.exit(f'no SRCS in the Makefile of {tree}')
    return tuple(m.group(1).replace('\\\n', ' ').split())


def disasm(tree, unit, out):
    obj = os.path.join(out, unit + '.co')
    src = os.path.join(tree, 'gym-soccer-2d-env_amd', 'csrc', unit)
    subprocess.run([HIPCC] + FLAGS + ['-c', '-o', obj, src], check=True)
    txt = subprocess.run([OBJDUMP, '-d', '--no-show-raw-insn', obj], check=True, capture_output=True, text=True).stdout
    funcs, cur, since_pc = {}, None, 9
    for line in txt.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith('\t'):
            continue
        ins = re.sub(r'<[^>]*>', '', line.split('//')[0]).strip()
        since_pc = 0 if ins.startswith('s_getpc') else since_pc + 1
        if since_pc <= 2 and ins.startswith(('s_add_u32', 's_addc_u32')):      # PC-relative literal of a code-object address
            ins = re.sub(r'0x[0-9a-fA-F]+|\b-?\d+$', 'X', ins)
        if ins and ins not in ('s_nop 0', '...'):                                # '...': objdump's run of zero padding
            cur.append(' '.join(ins.split()))
    for f in funcs.values():
        while f and f[-1] in ('s_code_end', 's_nop 0'):
            f.pop()
    return {k: v for k, v in funcs.items() if v}


def demangled(syms):
    out = subprocess.run(['c++filt'] + list(syms), check=True, capture_output=True, text=True).stdout
    return dict(zip(syms, out.splitlines()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--rename', action='append', default=[], help='OLD_SYM=NEW_SYM')
    ap.add_argument('--new-template-arg', action='append', default=[], help='text of a template argument only the new symbols have')
    a = ap.parse_args()
    ren = dict(r.split('=', 1) for r in a.rename)
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units(a.new):
            os.makedirs(os.path.join(tmp, 'old'), exist_ok=True)
            os.makedirs(os.path.join(tmp, 'new'), exist_ok=True)
            in_old = os.path.exists(os.path.join(a.old, 'gym-soccer-2d-env_amd', 'csrc', unit))   # a unit the new tree adds
            old = disasm(a.old, unit, os.path.join(tmp, 'old')) if in_old else {}
            new = disasm(a.new, unit, os.path.join(tmp, 'new'))
            if a.new_template_arg and old and new:
                dold, dnew = demangled(sorted(old)), demangled(sorted(new))
                for nsym, name in dnew.items():
                    for text in a.new_template_arg:
                        name = name.replace(text, '', 1)                # its first occurrence: the template argument list
                    for osym, oname in dold.items():
                        if oname == name and osym not in new:
                            ren[osym] = nsym
            for sym in sorted(old):
                nsym = ren.get(sym, sym)
                if nsym not in new:
                    print(f'gone {len(old[sym])} {unit} {sym}')
                    differ += 1
                    continue
                same = old[sym] == new[nsym]
                differ += not same
                tag = 'identical' if same else 'DIFFERENT'
                print(f'{tag} {len(old[sym])} {len(new[nsym])} {unit} {sym}' + (f' -> {nsym}' if nsym != sym else ''))
            for sym in sorted(set(new) - {ren.get(s, s) for s in old}):
                mf = sum(1 for i in new[sym] if i.startswith('v_mfma'))
                print(f'new {len(new[sym])} {unit} {sym} ({mf} v_mfma)')
    sys.exit(1 if differ else 0)


if __name__ == '__main__':
    main()
