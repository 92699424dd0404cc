"""The dense rule of the all-far tile program, checked on the built library's ISA (no GPU needed): every MFMA of the dense program is
issued.  The groups of the all-far program whose products are +-0 or discarded take loop-invariant operands from registers (DESIGN.md
3.1, "held operands"), and the MFMA builtin is pure: a compiler that hoists such a group out of its loop, or merges two of them,
leaves fewer `v_mfma` instructions in the kernel.  The full evaluation kernels carry three tile programs of 8 904 MFMAs each."""
import os
import re
import subprocess
import tempfile

import pytest

LLVM = '/opt/rocm/lib/llvm/bin'
MFMA_PER_PROGRAM = 8904
# k_field2_hand_f16<1>: counted in the disassembly of the parent commit's build (a7000bd, "all-far tiles stop fetching the weights of
# zero products") with this file's own count_mfma, which gives 26 712 = 3 x 8 904 for k_field2_hand<1> of the same build -- three
# programs of 5 320: the hidden layers and the reverse sweep run one pass per product
F16_PARENT_COUNT = 15960


@pytest.fixture(scope='module')
def built_lib():
    from honerf_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib


def count_mfma(lib_path, kernels):
    """-> {demangled kernel name: number of v_mfma instructions} for the gfx950 code objects of the library that define `kernels`"""
    out = {}
    with tempfile.TemporaryDirectory() as T:
        subprocess.run(['cp', lib_path, os.path.join(T, 'x.so')], check=True)
        subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', 'x.so'], cwd=T, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for f in sorted(os.listdir(T)):
            if 'gfx950' not in f or b'k_field2_hand' not in open(os.path.join(T, f), 'rb').read():
                continue
            dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', os.path.join(T, f)], check=True, capture_output=True, text=True).stdout
            for fn in re.split(r'\n(?=[0-9a-f]{16} <)', dis):
                m = re.match(r'[0-9a-f]{16} <(\S+)>:', fn)
                if not m:
                    continue
                # Itanium mangling of hn::v2::NAME<MODE>(Hand2Args): ... <length>NAME ILi<MODE>EE ...
                k = re.search(r'\d+(k_field2_hand\w*?)ILi(\d+)EE', m.group(1))
                name = '%s<%s>' % k.groups() if k else None
                if name in kernels:
                    assert name not in out, 'two definitions of %s' % name
                    out[name] = len(re.findall(r'\bv_mfma_', fn))
    return out


def test_the_full_evaluation_kernels_keep_every_mfma(built_lib):
    got = count_mfma(built_lib.LIB_PATH, ('k_field2_hand<1>', 'k_field2_hand_f16<1>'))
    assert got == {'k_field2_hand<1>': 3 * MFMA_PER_PROGRAM, 'k_field2_hand_f16<1>': F16_PARENT_COUNT}, got
