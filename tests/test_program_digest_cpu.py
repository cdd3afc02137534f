"""Every compiled Program, byte for byte, without a GPU: the programs of tests/program_digest_cases.py are built and one short
sha256 digest per field (op arrays, problem table, index blob, data-parallel parts, scheduling and layout fields, both states of
the tile-gradient route switch) is compared with the literals recorded there from the commit before the backward build was cut
into stages.  A changed digest is a changed program; the assertion names the fields that moved.

About 200 compiles of 10-40 ms: the module's 199 tests took 5.9, 6.5 and 8.0 s in three runs on a CPU (the last beside other
work)."""
import os

import pytest

import program_digest_cases as D


@pytest.fixture
def no_switches(monkeypatch):
    for k in [k for k in os.environ if k.startswith('GHN3_')]:
        monkeypatch.delenv(k)
    return monkeypatch


def test_every_case_has_its_literal_and_every_literal_its_case():
    assert set(D.EXPECT) == set(D.CASES)
    for name, line in D.EXPECT.items():
        assert len(line.split()) == len(D.FIELDS), name


def test_every_switch_case_differs_from_its_base_program():
    cases = [n for n in D.CASES if n.startswith('switch/')]
    assert len(cases) >= 35
    for name in cases:
        assert D.EXPECT[name] != D.EXPECT[D.switch_base(name)], name


@pytest.mark.parametrize('name', list(D.CASES))
def test_the_program_compiles_to_the_recorded_bytes(no_switches, name):
    prog = D.build(name, no_switches.setenv, no_switches.setattr)
    got = D.digests(prog)
    want = dict(zip(D.FIELDS, D.EXPECT[name].split()))
    print(' '.join(got.values()))
    moved = [f for f in D.FIELDS if got[f] != want[f]]
    assert not moved, 'fields that differ from the recorded program: %s' % moved
