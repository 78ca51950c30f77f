#!/usr/bin/env python3
'''Generates the Sobol direction table of mod16_amd/csrc/mod16_sobol.hpp (the block between the
"BEGIN/END SOBOL TABLE" markers) from scipy's unscrambled sequence:

  V[k][b] = point 2^(b+1) - 1 of scipy.stats.qmc.Sobol(32, scramble=False, bits=32), dimension k,
            times 2^32 (the Gray code of 2^(b+1) - 1 is 2^b, so that point IS direction number b)

  python tools/make_sobol_table.py          prints the block
  python tools/make_sobol_table.py --write  rewrites it in the header

tests/test_sensitivity_host.py checks that the committed block equals derive().'''
import os
import re
import sys

DIMS = 32
BITS = 32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      'mod16_amd', 'csrc', 'mod16_sobol.hpp')
BEGIN = '// BEGIN SOBOL TABLE (tools/make_sobol_table.py)'
END = '// END SOBOL TABLE'


def derive():
    '''V as a list of DIMS lists of BITS ints.'''
    import numpy as np
    from scipy.stats import qmc
    eng = qmc.Sobol(DIMS, scramble=False, bits=BITS)
    table = np.zeros((DIMS, BITS), np.uint64)
    for b in range(BITS):
        eng.reset()
        eng.fast_forward(2 ** (b + 1) - 1)
        table[:, b] = (eng.random(1)[0] * 2.0 ** BITS).astype(np.uint64)
    return [[int(v) for v in row] for row in table]


def render(table):
    lines = [BEGIN, 'static __constant__ uint32_t kSobolV[%d][%d] = {' % (DIMS, BITS)]
    for row in table:
        words = ['0x%08xu' % v for v in row]
        lines.append('    {' + ', '.join(words[:8]) + ',')
        for at in (8, 16):
            lines.append('     ' + ', '.join(words[at:at + 8]) + ',')
        lines.append('     ' + ', '.join(words[24:]) + '},')
    lines += ['};', END]
    return '\n'.join(lines)


def committed(path=HEADER):
    '''The table in the header, parsed back (a list of DIMS lists of BITS ints).'''
    text = open(path).read()
    block = text[text.index(BEGIN):text.index(END)]
    body = block[block.index('= {'):]
    words = [int(w, 16) for w in re.findall(r'0x([0-9a-f]{8})u', body)]
    return [words[k * BITS:(k + 1) * BITS] for k in range(len(words) // BITS)]


if __name__ == '__main__':
    block = render(derive())
    if '--write' in sys.argv:
        text = open(HEADER).read()
        a, b = text.index(BEGIN), text.index(END) + len(END)
        with open(HEADER, 'w') as f:
            f.write(text[:a] + block + text[b:])
    else:
        print(block)
