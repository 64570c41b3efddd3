"""Every DD_* knob the library reads has a test of its alternate path: the once-per-process
knobs of the conv family in the setting table of tests/test_gpu_conv_knobs.py (one child
process per setting), every other knob in the list below, paired with the existing test file
that toggles it.  A new knob cannot land without one or the other."""
import os
import re

import test_gpu_conv_knobs as conv_knobs
from test_knobs_documented import ROOT, _csrc_files, _library_knobs, _read

# knob -> the test file that sets it (per-call knobs by monkeypatch, DD_SELECT_RANK in a child)
TOGGLED_IN = {
    "DD_PEGRAD_WIDE": "tests/test_gpu_pegrad_wide.py",
    "DD_BN_QUAD": "tests/test_gpu_el2n_fast.py",
    "DD_C1_ROWQ": "tests/test_gpu_conv1x1.py",
    "DD_CONV_PW": "tests/test_gpu_pipeline.py",
    "DD_DOWN_PW": "tests/test_gpu_pipeline.py",
    "DD_PGQ": "tests/test_gpu_kernels.py",
    "DD_SELECT_RANK": "tests/test_gpu_select.py",
}


def test_every_library_knob_has_a_test_of_its_alternate_path():
    lib = _library_knobs()
    assert lib, "the collector found nothing: the pattern no longer matches the code"
    in_table = {k for k, _, _ in conv_knobs.SETTINGS}
    assert not in_table & set(TOGGLED_IN)
    assert lib == in_table | set(TOGGLED_IN), sorted(lib ^ (in_table | set(TOGGLED_IN)))


def test_the_listed_files_set_their_knobs():
    for knob, rel in TOGGLED_IN.items():
        text = _read(os.path.join(ROOT, rel))
        assert f'setenv("{knob}"' in text or f'{knob}="' in text, (knob, rel)


def _library_defaults():
    """knob -> the set of defaults its env_int calls give (literal text: a number or a name)."""
    out = {}
    for path in _csrc_files():
        for name, dflt in re.findall(r'\benv_int\(\s*"(\w+)"\s*,\s*([\w-]+)\s*\)', _read(path)):
            out.setdefault(name, set()).add(dflt)
    return out


def test_every_setting_differs_from_the_default():
    """The table holds non-default values only, the defaults being those of the env_int calls
    in the sources.  A knob read with two defaults (DD_DOWN_XCD: forward 2, backward 1) has each
    of them in the table, as the alternate of the other reader."""
    defaults = _library_defaults()
    for knob, value, _ in conv_knobs.SETTINGS:
        assert defaults[knob] != {value}, (knob, value)
    for knob in {k for k, _, _ in conv_knobs.SETTINGS}:
        if len(defaults[knob]) > 1:
            assert defaults[knob] <= {v for k, v, _ in conv_knobs.SETTINGS if k == knob}, knob
