"""Every once-per-process DD_* knob of the conv family: the family's
launch list (tests/helpers/conv_launches.py) run in a child process under each non-default
setting gives bitwise the outputs of a child run with nothing set -- tensors, fragment-mask
words, plane bits and the raw BN partial statistics alike.  The one exception: under
DD_C1_EPI=0 and DD_DOWN_EPI=0 the statistics partials of exactly the launches whose kernel the
knob swaps (Launch.epi_stats) differ in their last bits and are held to float64 instead
(STATS_BY_FINALIZE below; profiles/conv_matrix/README.md).

The knobs are read once per process, so each setting is a child of its own
(tests/helpers/conv_knob_child.py), one at a time, each under its own timeout.  A child that
fails in any way (a signal, its timeout, or a non-zero exit, which is how a HIP error raised
as a Python exception ends it) stops the module: no further child is started and the remaining
cases fail with that reason.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (knob, value, family whose list runs under it)
SETTINGS = [
    ("DD_CONV_XCD", "0", "conv3x3"),
    ("DD_CONV_EPI", "0", "conv3x3"),
    ("DD_DOWN_WA", "2", "down"),
    ("DD_DOWN_EPI", "0", "down"),
    ("DD_DOWN_BWD", "1", "down"),
    ("DD_DOWN_XCD", "0", "down"),
    ("DD_DOWN_XCD", "1", "down"),
    ("DD_DOWN_XCD", "2", "down"),
    ("DD_C1_FAMILY", "1", "c1x1"),
    ("DD_C1_FAMILY", "2", "c1x1"),
    ("DD_C1_FAMILY", "3", "c1x1"),
    ("DD_C1_EPI", "0", "c1x1"),
    ("DD_C1_XCD", "0", "c1x1"),
    ("DD_C1_XCD", "1", "c1x1"),
]
# Not bit-neutral for the raw statistics partials: the 1x1 kernel leaves its sums of squares to
# the compiler's contraction, which fuses them in the specialised epilogues (v_fmac, the first
# two squares of a row joined in the other order) and not in the run-time-flag kernel (v_mul +
# v_pk_add), so the partials differ in their last bits.  Every other output stays bitwise equal,
# and both runs' partials must meet the float64 group statistics through bn_finalize.
# The downsampling head's epilogue has the same source pattern (q_ += us * us under a
# compile-time or a run-time flag), and its generated code differs the same way.  Only the
# launches whose kernel the knob swaps are exempt (Launch.epi_stats names the knob: the
# shortcut-fused statistics launch of the head, the float4 1x1 statistics launches).
STATS_BY_FINALIZE = {("DD_C1_EPI", "0"), ("DD_DOWN_EPI", "0")}
STATS_KEYS = {"stats": "_st", "stats_sc": "_sts"}  # raw partials -> the launch's BNStats
KNOBS = sorted({k for k, _, _ in SETTINGS})
FAMILIES = sorted({f for _, _, f in SETTINGS})
CHILD_TIMEOUT = 180  # seconds; a child takes a few (start-up included)

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "helpers", "conv_knob_child.py")
_dead = []  # why the module starts no further child


def _child(family, setting, path):
    if _dead:
        pytest.fail(f"no further child after: {_dead[0]}")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(setting)
    what = f"{family} child under {setting or 'defaults'}"
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, CHILD, family, path], env=env, capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append(f"{what} ran into its {CHILD_TIMEOUT} s timeout")
        pytest.fail(_dead[0])
    if r.returncode != 0 or "child ok" not in r.stdout:
        how = f"ended on signal {-r.returncode}" if r.returncode < 0 else f"exited {r.returncode}"
        _dead.append(f"{what} {how}: {r.stdout[-500:]}{r.stderr[-3000:]}")
        pytest.fail(_dead[0])
    print(f"CHILD {what}: {r.stdout.strip().splitlines()[-1]}; wall {time.time() - t0:.1f} s")
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def default_runs(cuda, tmp_path_factory):
    """Each family's list under the default settings, once."""
    d = tmp_path_factory.mktemp("conv_knobs")
    return {f: _child(f, {}, str(d / f"{f}_default.npz")) for f in FAMILIES}


@pytest.mark.parametrize("knob,value,family", SETTINGS, ids=[f"{k}={v}" for k, v, _ in SETTINGS])
def test_setting_is_bit_neutral(cuda, default_runs, tmp_path, knob, value, family):
    from helpers import conv_launches as cl

    base = default_runs[family]
    got = _child(family, {knob: value}, str(tmp_path / "run.npz"))
    refused = {la.name for la in cl.launches(family) if la.skip_env.get(knob) == value}
    want_keys = {k for k in base if k.split("/")[0] not in refused}
    assert set(got) == want_keys
    diff = [k for k in sorted(got) if not np.array_equal(got[k], base[k])]
    if (knob, value) in STATS_BY_FINALIZE:
        swapped = {la.name for la in cl.launches(family) if la.epi_stats == knob}
        assert swapped
        for key in [k for k in diff
                    if k.split("/")[0] in swapped and k.split("/")[1] in STATS_KEYS]:
            _stats_meet_float64(cuda, cl, *key.split("/"), (base[key], got[key]))
            diff.remove(key)
    assert not diff, f"{len(diff)} of {len(got)} outputs differ under {knob}={value}: {diff[:12]}"


def _stats_meet_float64(cuda, cl, name, out_key, raws):
    """Both runs' raw partials of one launch, through bn_finalize, against the float64 group
    statistics at the tolerance of tests/test_gpu_conv_matrix.py."""
    import torch

    from data_diet_distributed_amd import _capi
    from test_gpu_conv_matrix import STAT_REL, _close

    la = next(x for x in cl.LAUNCHES if x.name == name)
    inp = la.inputs()
    out = la.run(inp, cuda)  # the BNStats geometry of the launch
    st_key, y_key, gs, nst = next(s for s in la.stats if s[0] == STATS_KEYS[out_key])
    st = out[st_key]
    rsc, rsh = cl.group_bn_ref(la.ref(inp, out)[y_key][0], gs, nst, inp["gamma"], inp["beta"])
    for raw in raws:
        assert raw.size == st.buf.numel() * 4
        st.buf = torch.from_numpy(raw.copy()).view(torch.float32).to(cuda)
        sc, sh = _capi.bn_finalize(st, inp["gamma"].to(cuda), inp["beta"].to(cuda), cl.EPS)
        _close(sc, rsc, STAT_REL[la.operands])
        _close(sh, rsh, STAT_REL[la.operands])
