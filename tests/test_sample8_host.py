"""The device's 8-of-M sampler (mvslam_amd/csrc/sampler.hpp) compiled for the host and compared with the oracle's sampler:
M in {8, 9, 10, 64, 1576, 4096, 2^24 - 1} x hypotheses 0 .. 4095 x three seeds, all eight indices equal and in order
(tests/cpp/sample8_host.cpp).  The sample stream is contract: any reformulation of the
rank / insert network has to pass this.  No GPU needed; the second case is the same program under ASan + UBSan, stand-alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_device_sampler_matches_the_oracle_on_the_host(tmp_path, sanitize):
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    objs = []
    for name in ("mvs_oracle", "mvs_refine_oracle", "mvs_orb_oracle"):
        obj = str(tmp_path / (name + ".o"))
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-mfma", *san, "-c", os.path.join(ROOT, "oracle", name + ".c"),
                               "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "sample8_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", *san, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "sample8_host.cpp"), *objs, "-lm"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "sample8 checked=%d bad=0" % (7 * 3 * 4096) in out and "ERROR" not in out and "runtime error" not in out, out
