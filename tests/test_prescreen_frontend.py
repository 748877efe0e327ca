"""The pre-screen's front end (sampler, 32-bit gather offsets, Hartley normalisations without per-root fix-ups and their
guarded fall-back) against the oracle, hypothesis by hypothesis: tests/prescreen_frontend_gpu_check.py, in a process of
its own because the record reader lives in the diagnostics library."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(spread):
    env = dict(os.environ, MVS_USE_DEBUG_LIB="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "prescreen_frontend_gpu_check.py"), repr(spread)], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    st = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(st))
    return st


@pytest.mark.gpu
def test_front_end_records_and_states_with_zero_radicands():
    """3 pairs x 512 hypotheses, M = 33 / 9 / 8; pair 2's image-1 coordinates lie within 1e-200 of each other: every q of its
    samples underflows to 0, the guarded normalisation runs and rejects them (2 record layouts x 512 hypotheses)"""
    st = _run(1e-201)
    assert st["viol"] == 0 and st["count_viol"] == 0
    assert st["hyp"] == 2 * 3 * 512 and st["zero_q"] == 2 * 512 and st["tiny"] == 0
    assert st["invalid"] >= 2 * 512 and st["certified"] > 0            # pair 2 rejected; the general pair gets certificates
    assert st["valid"] == [1, 1, 0]


@pytest.mark.gpu
def test_front_end_records_and_states_with_tiny_radicands():
    """the same with a spread of 1e-130: 0 < q < 2^-767 -- the `tiny` decision: no certificate and no rejection by the
    pre-screen, the exact solve rejects the samples"""
    st = _run(1e-130)
    assert st["viol"] == 0 and st["count_viol"] == 0
    assert st["hyp"] == 2 * 3 * 512 and st["tiny"] == 2 * 512 and st["need_exact"] >= 2 * 512
    assert st["certified"] > 0
    assert st["valid"] == [1, 1, 0]
