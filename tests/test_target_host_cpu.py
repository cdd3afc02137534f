"""The host contract of the target-network convolution ops, pinned without a GPU: the sizes the seven `*_scratch_floats` functions
answer and the calls the twelve entry points refuse, against the literals of tests/target_host_cases.py (recorded from the library
before its host code was reorganised; the kernels themselves are tested in tests/test_gpu_target_*.py).

The library is asked in ONE child process that sees no GPU: every call here must return before its first HIP call, and one that
does not fails there at its first launch, with a HIP error in place of the recorded refusal, instead of running a kernel on the
dummy pointers."""
import json
import os
import subprocess
import sys

import pytest

import target_host_cases as H


@pytest.fixture(scope='module')
def answers():
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', ROCR_VISIBLE_DEVICES='')
    run = subprocess.run([sys.executable, H.__file__, '--json'], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    return json.loads(run.stdout)


def test_every_descriptor_and_call_has_its_literal(answers):
    for family, (_, descs, functions) in H.SIZE_FUNCTIONS.items():
        assert set(H.SIZES[family]) == set(descs) == set(answers['sizes'][family]), family
        assert all(set(row) == set(functions) for row in H.SIZES[family].values()), family
    cases = [c[0] for c in H.entry_calls()]
    assert len(cases) == len(set(cases)) and set(cases) == set(H.REFUSALS) == set(answers['refusals'])
    assert {c[1] for c in H.entry_calls()} == set(H.ENTRY)
    assert len(H.DWPW) >= 40 and len(H.CONV) >= 30


DESCRIPTORS = [(f, n) for f, (_, descs, _) in H.SIZE_FUNCTIONS.items() for n in descs]


@pytest.mark.parametrize('family,name', DESCRIPTORS, ids=['%s-%s' % fn for fn in DESCRIPTORS])
def test_scratch_sizes_and_their_refusals(answers, family, name):
    got, want = answers['sizes'][family][name], H.SIZES[family][name]
    print(got)
    assert got == want
    for fn, pair in got.items():
        for n in pair:                                              # (what holds whatever was recorded)
            if isinstance(n, list):
                assert n[0] in (-1, -2) and n[1].startswith(('dwpw: ', 'dw: ', 'conv: ', 'patch: ')), (fn, n)
                # the three size functions of the fused chain answer -1 whatever the reason; the others the code of the refusal
                assert n[0] == -1 or fn.startswith(('ghn3_dw_', 'ghn3_conv_', 'ghn3_patch_')), (fn, n)
            else:
                assert n % 4 == 0, (fn, n)                          # every area starts on 16 bytes
        assert isinstance(pair[0], list) == isinstance(pair[1], list), (fn, pair)      # a refusal does not depend on the direction


def test_sizes_of_the_members_differ_as_their_layouts_say(answers):
    """What ties the members' sizes together, for every descriptor all of them take."""
    for name, fields in H.DWPW.items():
        row = answers['sizes']['dwpw'][name]
        batch, plain, frozen, alone = (row['ghn3_dw%s_scratch_floats' % m] for m in ('pw', 'pw_plain', 'pw_frozen', ''))
        if isinstance(batch[1], list):
            assert isinstance(plain[1], list) and isinstance(frozen[1], list)
            continue
        C_out, P = fields[4], fields[0] * fields[9] * fields[10]
        tiles = (P + 63) // 64
        assert batch[0] == 2 * tiles * C_out + 64 and plain[0] == 0 and frozen[0] == 0
        assert batch[1] - plain[1] == 2 * tiles * C_out + 2 * C_out and frozen[1] - batch[1] == 2 * C_out
        if not isinstance(alone[1], list):
            assert alone[0] == 0 and 256 <= alone[1] <= plain[1]
    for name, fields in H.CONV.items():
        row = answers['sizes']['conv'][name]
        batch, frozen = row['ghn3_conv_scratch_floats'], row['ghn3_conv_frozen_scratch_floats']
        if isinstance(batch[1], list):
            assert frozen == batch
            continue
        C_out, P = fields[4], fields[0] * fields[12] * fields[13]
        assert batch[0] - frozen[0] == 2 * ((P + 63) // 64) * C_out and frozen[1] - batch[1] == 2 * C_out


@pytest.mark.parametrize('case', [c[0] for c in H.entry_calls()])
def test_entry_points_refuse(answers, case):
    got = answers['refusals'][case]
    print(got)
    assert got == H.REFUSALS[case]
    assert got[0] in (-1, -2), 'not refused before the first HIP call'


def test_the_spot_values_of_the_recording():
    s = H.SIZES['dwpw']['spot/n2_8x8_c32']
    assert [s[f] for f in H.SIZE_FUNCTIONS['dwpw'][2]] == [[192, 10944], [0, 10752], [0, 11008], [0, 2560]]
    s = H.SIZES['dwpw']['spot/n3_7x5_c4_c8_s2']
    assert [s[f] for f in H.SIZE_FUNCTIONS['dwpw'][2][:3]] == [[80, 604], [0, 572], [0, 620]]
    assert [n[0] for n in s['ghn3_dw_scratch_floats']] == [-1, -1]
    s = H.SIZES['conv']['spot/n2_9x9_c16_c24_3x1']
    assert [s[f] for f in H.SIZE_FUNCTIONS['conv'][2]] == [[3616, 8320], [3520, 8368]]
