"""Which gfx950 kernels of a .hip source changed between two git revisions?  Compiles both versions to assembly and compares the
instruction streams per kernel symbol (labels normalised).  Used to show that a refactor left the validated default kernels
bit-identical when there is no GPU time to re-run the suite.  A kernel whose stream differs is `reordered` (the same work in another
schedule) when its MFMA / LDS / vector-memory / scalar-load / barrier instruction counts, scratch, VGPR spills, static LDS size and
occupancy equal the old revision's and it is at most 1 % longer; anything else is `CHANGED`.  Exit status 1 on CHANGED or MISSING.

  python tools/isa_diff.py cat_amd/csrc/norm.hip [old_rev=HEAD~1] [new_rev=WORKTREE]"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def source_at(path, rev):
    if rev == 'WORKTREE':
        return open(os.path.join(ROOT, path)).read()
    return subprocess.run(['git', '-C', ROOT, 'show', f'{rev}:{path}'], check=True, capture_output=True, text=True).stdout


def kernels(src, path, tmp, tag):
    inc = os.path.join(ROOT, os.path.dirname(path))
    f = os.path.join(tmp, tag + '.hip')
    open(f, 'w').write(src)
    out = os.path.join(tmp, tag + '.s')
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', inc, '-S', '--offload-device-only',
                        '-Rpass-analysis=kernel-resource-usage', f, '-o', out], check=True, capture_output=True, text=True)
    text = open(out).read()
    for rec in re.split(r'\n  - (?=\.)', text[text.index('amdhsa.kernels:'):])[1:]:   # kernel descriptor metadata, as tools/codegen_table.py reads it
        g = lambda k: int(re.search(r'\.' + k + r':\s+(\d+)', rec).group(1))
        RES[tag, re.search(r'\n    \.name:\s+(\S+)', rec).group(1)] = {
            k: g(k) for k in ('private_segment_fixed_size', 'vgpr_spill_count', 'group_segment_fixed_size', 'sgpr_count', 'vgpr_count')}
    for m in re.finditer(r'Function Name: (\S+) .*?Occupancy \[waves/SIMD\]: (\d+)', r.stderr, re.S):
        RES.get((tag, m.group(1)), {})['occupancy'] = int(m.group(2))
    res, cur = {}, None
    for line in open(out):
        m = re.match(r'^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$', line)
        if m and not line.startswith('.'):
            cur = m.group(1)
            res[cur] = []
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith('s_endpgm'):
            cur = None
            continue
        if not t or t.startswith((';', '.')):
            continue
        res[cur].append(re.sub(r'\.LBB\d+_\d+', '.L', re.sub(r';.*', '', t)).strip())
    return {k: v for k, v in res.items() if v and not k.startswith('__hip_cuid')}


RES = {}   # (tag, symbol) -> resources the compiler reports
CLASSES = (('mfma', r'v_mfma'), ('lds', r'ds_'), ('vmem', r'(global|buffer|flat|scratch)_'), ('smem', r's_(buffer_)?load'), ('barrier', r's_barrier'))
FIXED = ('private_segment_fixed_size', 'vgpr_spill_count', 'group_segment_fixed_size', 'occupancy')


def counts(body):
    return tuple(sum(1 for t in body if re.match(pat, t)) for _, pat in CLASSES)


def base_name(sym):   # function name of an Itanium-mangled symbol, template arguments dropped
    pos, parts = 2 + sym.startswith('_ZN'), []
    while sym.startswith('_Z') and (m := re.match(r'\d+', sym[pos:])):
        pos += m.end() + int(m.group())
        parts.append(sym[pos - int(m.group()):pos])
    return '::'.join(parts) or sym


def judge(k_old, k_new, v, w):
    """verdict and detail for a kernel whose instruction stream differs (v: old body, w: new body)"""
    ro, rn = RES['old', k_old], RES['new', k_new]
    co, cn = counts(v), counts(w)
    ok = co == cn and all(ro[f] == rn[f] for f in FIXED) and len(w) * 100 <= len(v) * 101
    d = f'{len(v)} -> {len(w)} instructions ({(len(w) - len(v)) * 100.0 / len(v):+.2f} %); ' + ' '.join(
        f'{n} {a}' + ('' if a == b else f'->{b}') for (n, _), a, b in zip(CLASSES, co, cn))
    d += ''.join(f'; {f} {ro[f]}->{rn[f]}' for f in FIXED + ('sgpr_count', 'vgpr_count') if ro[f] != rn[f])
    return ok, d


def main():
    path = sys.argv[1]
    old_rev = sys.argv[2] if len(sys.argv) > 2 else 'HEAD~1'
    new_rev = sys.argv[3] if len(sys.argv) > 3 else 'WORKTREE'
    with tempfile.TemporaryDirectory() as tmp:
        with ThreadPoolExecutor(2) as ex:   # the two compiles side by side
            old, new = ex.map(lambda a: kernels(source_at(path, a[0]), path, tmp, a[1]), ((old_rev, 'old'), (new_rev, 'new')))
    return report(old, new)


def report(old, new):
    same = reordered = changed = 0
    new_by_body = {}
    for k, v in new.items():
        new_by_body.setdefault(tuple(v), []).append(k)
    fresh = sorted(set(new) - set(old))
    for k, v in sorted(old.items()):
        twins = [k] if new.get(k) == v else [] if k in new else new_by_body.get(tuple(v))
        # a renamed kernel whose body moved as well: the one new symbol of the same function name, if the old name has one unmatched too
        cand = [n for n in fresh if base_name(n) == base_name(k)] if k not in new else [k]
        if twins:
            print('identical ' + k + (f'  (now {twins[0]})' if twins[0] != k else ''))
            same += 1
        elif len(cand) == 1 and (k in new or sum(1 for o in old if o not in new and base_name(o) == base_name(k)) == 1):
            ok, detail = judge(k, cand[0], v, new[cand[0]])
            print(('reordered ' if ok else 'CHANGED   ') + k + (f'  (now {cand[0]})' if cand[0] != k else '') + '  (' + detail + ')')
            reordered += ok
            changed += not ok
        else:
            print('MISSING   ' + k)
            changed += 1
    for k in fresh:
        print('new       ' + k)
    print(f'{same} identical, {reordered} reordered, {changed} changed / missing, {len(fresh)} new symbols')
    return 1 if changed else 0


if __name__ == '__main__':
    sys.exit(main())
