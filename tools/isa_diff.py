#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two gfx950 device-assembly files (hipcc -save-temps=obj:
<source>-hip-amdgcn-amd-amdhsa-gfx950.s), for refactors that must not change the generated code.

    python tools/isa_diff.py before.s after.s [--rename 's/REGEX/REPL/' ...]

A kernel is its instruction stream plus its .amdhsa_kernel descriptor block.  Local label numbers (.LBB<n>_) are
normalised and comments dropped, nothing else; --rename rewrites mangled names on both sides first (a dropped template parameter).
A kernel that differs is listed with what the compiler reports for it on either side.
Exit status 0: same set of kernels, all identical."""
import re
import sys


RES = {}      # (file, kernel) -> the registers / scratch / LDS / occupancy / code size the compiler reports


def kernels(path, renames):
    """{kernel: [lines]}: the text between `<name>:` and its .Lfunc_end, then the .amdhsa_kernel block."""
    text = open(path).read()
    for pat, rep in renames:
        text = re.sub(pat, rep, text)
    names = re.findall(r'^\s*\.amdhsa_kernel (\S+)', text, flags=re.M)
    out = {}
    for name in names:
        body = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:' % re.escape(name), text, flags=re.M | re.S).group(1)
        desc = re.search(r'^\s*\.amdhsa_kernel %s\n(.*?)^\s*\.end_amdhsa_kernel' % re.escape(name), text, flags=re.M | re.S).group(1)
        lines = [re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].strip()) for ln in (body + desc).splitlines()]
        out[name] = [ln for ln in lines if ln]
        info = text[text.index('; Kernel info:', text.index('.Lfunc_end', text.index('\n%s:' % name))):]      # the block after the body
        RES[path, name] = ' '.join('%s=%s' % (k, re.search(r'^; %s:? =? ?(\d+)' % k, info, flags=re.M).group(1))
                                   for k in ('NumVgprs', 'ScratchSize', 'LDSByteSize', 'Occupancy', 'codeLenInByte'))
    return out


def main(argv):
    renames = []
    while '--rename' in argv:
        i = argv.index('--rename')
        _, pat, rep, _ = argv[i + 1].split('/')
        renames.append((pat, rep))
        del argv[i:i + 2]
    before, after = kernels(argv[1], renames), kernels(argv[2], renames)
    bad = 0
    for name in sorted(set(before) | set(after)):
        if name not in before or name not in after:
            print('ONLY IN %s  %s' % ('before' if name in before else 'after ', name))
            bad += 1
        elif before[name] != after[name]:
            n = next((i for i, (x, y) in enumerate(zip(before[name], after[name])) if x != y), min(len(before[name]), len(after[name])))
            print('DIFFERENT    %s  (%d / %d lines, first difference at line %d)' % (name, len(before[name]), len(after[name]), n))
            print('      before %s\n      after  %s' % (RES[argv[1], name], RES[argv[2], name]))
            bad += 1
        else:
            print('identical    %s  (%d lines)' % (name, len(before[name])))
    print('%d kernels before, %d after, %d not identical' % (len(before), len(after), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
