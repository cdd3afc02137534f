"""DESIGN.md's "Environment switches" table lists every GHN3_* variable the library reads (a text scan of the sources: a switch
that is added without a row, or a row-less leftover of a retired experiment, fails here)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r'''["'](GHN3_[A-Z0-9_]+)["']'''


def _names(pattern, reads):
    found = set()
    for path in sorted(glob.glob(os.path.join(ROOT, pattern))):
        with open(path, encoding='utf-8') as fh:
            found.update(re.findall(reads + r'\s*' + NAME, fh.read()))
    return found


def test_every_switch_the_library_reads_has_a_row_in_the_design_table():
    read = _names('ghn3_amd/*.py', r'os\.environ(?:\.get\(|\[)') | _names('ghn3_amd/csrc/*', r'getenv\(')
    assert len(read) > 40, sorted(read)                 # (the scan itself still finds the reads)
    with open(os.path.join(ROOT, 'DESIGN.md'), encoding='utf-8') as fh:
        text = fh.read()
    table = text[text.index('## Environment switches'):].split('\n## ')[0]
    rows = [ln for ln in table.splitlines()[1:] if ln.startswith('|')]
    listed = set(re.findall(r'`(GHN3_[A-Z0-9_]+)`', '\n'.join(ln.split('|')[1] for ln in rows)))
    assert not read - listed, 'switches without a row in DESIGN.md: %s' % sorted(read - listed)
