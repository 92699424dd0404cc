#!/usr/bin/env python3
"""Device code of two builds, symbol for symbol: tools/device_code_diff.py PARENT_BUILD_DIR NEW_BUILD_DIR

For every *.o of the two directories the gfx950 code object is taken out (llvm-objdump --offloading), disassembled
(llvm-objdump -d --no-leading-addr --no-show-raw-insn), split per symbol and compared as text.  One line per symbol: `equal (N lines)`
or `DIFFERENT`, with the symbol's vgpr / agpr / spill / scratch notes (llvm-readelf --notes) of both sides; the last line is
`== N symbols compared, M different`.  Exit status 1 if M > 0 or the two builds do not define the same symbols.  Host only; needs the
ROCm LLVM tools ($ROCM_PATH/lib/llvm/bin, default /opt/rocm)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin')


def tool(name, *args, **kw):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, capture_output=True, text=True, **kw).stdout


def device_code(obj):
    """-> {mangled symbol: (disassembly lines, resource note, demangled name)} of the object's gfx950 code object ({} if it has none)"""
    with tempfile.TemporaryDirectory() as T:
        shutil.copy(obj, os.path.join(T, 'x.o'))
        tool('llvm-objdump', '--offloading', 'x.o', cwd=T)
        cos = sorted(f for f in os.listdir(T) if 'gfx950' in f)
        if not cos:
            return {}
        co = os.path.join(T, cos[0])
        notes = {}
        for blk in tool('llvm-readelf', '--notes', co).split('- .agpr_count:')[1:]:
            def g(key):
                m = re.search(r'\.' + key + r':\s*(\S+)', blk)
                return m.group(1) if m else '?'
            notes[g('name')] = 'vgpr %s agpr %s spill %s scratch %s B' % (g('vgpr_count'), blk.split()[0], g('vgpr_spill_count'), g('private_segment_fixed_size'))
        # (the demangler at hand is llvm-objdump's own: the symbol table twice, line for line)
        plain, pretty = (tool('llvm-objdump', '-t', *opt, co).splitlines() for opt in ((), ('-C',)))
        names = {a.split()[-1]: re.sub(r'^\.\w+ ', '', b.split('\t')[-1].split(' ', 1)[-1]) for a, b in zip(plain, pretty) if '\t' in a}
        out = {}
        dis = tool('llvm-objdump', '-d', '--no-leading-addr', '--no-show-raw-insn', co)
        dis = re.sub(r'// [0-9A-F]{12}: ', '// ', dis)   # (the address in an instruction's comment: a symbol's text does not depend on where it lies)
        for fn in re.split(r'\n(?=<\S+>:\n)', dis):
            m = re.match(r'<(\S+)>:\n', fn)
            if m:
                out[m.group(1)] = (fn[m.end():].splitlines(), notes.get(m.group(1), 'no notes'), names.get(m.group(1), m.group(1)))
        return out


def main(parent_dir, new_dir):
    objs = [sorted(f for f in os.listdir(d) if f.endswith('.o')) for d in (parent_dir, new_dir)]
    total = different = 0
    sets_differ = objs[0] != objs[1]
    for o in sorted(set(objs[0]) & set(objs[1])):
        old, new = device_code(os.path.join(parent_dir, o)), device_code(os.path.join(new_dir, o))
        print('== %s: %d symbols in the parent, %d here' % (o, len(old), len(new)))
        for sym in old:
            shown = old[sym][2] if old[sym][2].startswith('hn::(') else old[sym][2].split('(')[0]
            if sym not in new:
                continue
            total += 1
            same = old[sym][:2] == new[sym][:2]
            different += not same
            if same:
                print('%-72.70s equal (%d lines)   [%s]' % (shown, len(old[sym][0]), old[sym][1]))
            else:
                print('%-72.70s DIFFERENT (%d / %d lines)   [parent: %s]   [here: %s]' % (shown, len(old[sym][0]), len(new[sym][0]), old[sym][1], new[sym][1]))
        for sym in sorted(set(old) ^ set(new)):
            sets_differ = True
            print('%-72.70s only in %s' % (sym, 'the parent' if sym in old else 'this build'))
    for o in sorted(set(objs[0]) ^ set(objs[1])):
        print('== %s: only in %s' % (o, 'the parent' if o in objs[0] else 'this build'))
    print('== %d symbols compared, %d different%s' % (total, different, ', the symbol sets differ' if sets_differ else ''))
    return 1 if different or sets_differ else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
