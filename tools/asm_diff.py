"""Is the device code of the kernels unchanged?  Compiles every HIP source of passl_amd/csrc at a given commit and in
the working tree to gfx950 assembly (same flags as the build) and compares the instruction streams kernel by kernel
(comments, debug lines and basic-block label numbers ignored).  A kernel whose name is gone while a new name carries
its instruction stream unchanged is reported as renamed, not as changed.  The compared stream runs to the end of the
kernel's descriptor (kernarg size, register counts), and the offsets of the hidden arguments follow the explicit ones:
a kernel folded into a template with another parameter list therefore comes out as removed + new, never as renamed.
A removed kernel is shown next to the new kernel whose stream is closest to it, with the number of lines that differ and
the opcodes whose counts changed: a rewrite that only moved instructions shows up as such.
Runs without a GPU.

    python tools/asm_diff.py <commit>        # e.g. the last commit whose build passed the GPU suite

Used to show that an opt-in kernel added next to the product kernels (a new template parameter with a default, a new
kernel in the same file) left the product kernels' code bit-identical."""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from passl_amd.csrc import build as B          # noqa: E402


def kernels(path):
    out, cur, buf = {}, None, []
    for line in open(path).read().split('\n'):
        m = re.match(r'^(_Z[\w$.]+):', line)
        if m and cur is None:
            cur, buf = m.group(1), []
            continue
        if cur is not None:
            if re.match(r'^\.Lfunc_end\d+:', line):
                out[cur] = buf
                cur = None
                continue
            s = re.sub(r'\s*;.*$', '', line).rstrip()
            if s.strip() and not s.strip().startswith(('.loc', '.file', '.cfi')):
                # (the kernel's own name, which its descriptor and section lines carry: a rename alone is no change)
                buf.append(re.sub(r'\.LBB\d+_', '.LBB_', s).replace(cur, '<kernel>'))
    return out


def assemble(src, dst):
    cmd = [B.hipcc()] + B.FLAGS + ['--cuda-device-only', '-S', src, '-o', dst]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])


def match(a, b):
    """{name: stream} of the old and the new build -> (different, renamed {old: new}, removed, new).  Renamed: the old
    name is gone and a new name carries its instruction stream unchanged (a kernel folded into a template, say)."""
    diff = [n for n in a if n in b and a[n] != b[n]]
    new = [n for n in b if n not in a]
    renamed = {}
    for n in a:
        twin = [k for k in new if n not in b and k not in renamed.values() and b[k] == a[n]]
        if twin:
            renamed[n] = twin[0]
    gone = [n for n in a if n not in b and n not in renamed]
    return diff, renamed, gone, [n for n in new if n not in renamed.values()]


def closest(stream, new):
    """(name, differing lines, {opcode: count change}) of the stream of `new` ({name: stream}) nearest to `stream`."""
    def opcodes(x):
        return collections.Counter(line.split()[0] for line in x if line.startswith('\t') and not line.lstrip().startswith('.'))
    name = max(new, key=lambda k: difflib.SequenceMatcher(None, stream, new[k], autojunk=False).ratio())
    ops = difflib.SequenceMatcher(None, stream, new[name], autojunk=False).get_opcodes()
    lines = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != 'equal')
    a, b = opcodes(stream), opcodes(new[name])
    return name, lines, {o: b[o] - a[o] for o in sorted(set(a) | set(b)) if a[o] != b[o]}


def demangle(name):
    return subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()[:140]


def main():
    commit = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, 'old')
        os.makedirs(old)
        tar = subprocess.run(['git', '-C', ROOT, 'archive', commit, 'passl_amd/csrc', 'include'], capture_output=True, check=True)
        subprocess.run(['tar', '-x', '-C', old], input=tar.stdout, check=True)
        print('# device code of passl_amd/csrc at %s against the working tree (%s %s)' % (commit, os.path.basename(B.hipcc()), ' '.join(B.FLAGS)))
        changed = 0
        for s in B.SOURCES:
            po = os.path.join(old, 'passl_amd', 'csrc', s)
            if not os.path.exists(po):
                print('%-24s new file' % s)
                continue
            assemble(po, os.path.join(tmp, 'a.s'))
            assemble(os.path.join(B.HERE, s), os.path.join(tmp, 'b.s'))
            a, b = kernels(os.path.join(tmp, 'a.s')), kernels(os.path.join(tmp, 'b.s'))
            diff, renamed, gone, new = match(a, b)
            changed += len(diff) + len(gone)
            print('%-24s %3d kernels: %3d identical, %d renamed, %d different, %d removed, %d new'
                  % (s, len(a), len(a) - len(diff) - len(gone) - len(renamed), len(renamed), len(diff), len(gone), len(new)))
            for n, k in renamed.items():
                print('    renamed   %s -> %s' % (demangle(n), demangle(k)))
            for tag, names in (('different', diff), ('removed', gone), ('new', new)):
                for n in names:
                    print('    %-9s %s' % (tag, demangle(n)))
                    if tag == 'removed' and new:
                        k, lines, ops = closest(a[n], {x: b[x] for x in new})
                        print('              closest new: %s; %d of %d lines differ; opcode counts %s' % (
                            demangle(k), lines, len(a[n]), ', '.join('%s %+d' % kv for kv in ops.items()) or 'equal'))
        print('# %s' % ('every kernel of the old build is unchanged' if changed == 0 else '%d kernels changed' % changed))


if __name__ == '__main__':
    main()
