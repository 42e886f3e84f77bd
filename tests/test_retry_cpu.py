"""The retained-scratch policy of the prediction paths (csrc/ace_retry.h: run,
on out-of-memory recover and run once more, then trim) through
tests/retry_check.cpp, under AddressSanitizer + UBSan.  No GPU test can make
an allocation fail on a shared machine, so this is the out-of-memory path's
test; ace_predict.cpp's with_pred_scratch runs the function checked here.
CPU only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "additivecausalexpansion_amd", "csrc")


def test_retry_policy_is_sanitizer_clean(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no host compiler")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "retry_check")
    subprocess.run([gxx, *flags, "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "retry_check.cpp"), "-o", exe], check=True)
    # verify_asan_link_order=0: the process environment may preload other
    # libraries ahead of the ASan runtime; that is not a finding
    env = dict(os.environ,
               ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "retry_check: OK" in out.stdout


def test_prediction_paths_share_the_checked_policy():
    """The library runs the checked function, not a copy: ace_predict.cpp
    catches no out-of-memory failure of its own, every scratch user goes
    through the one wrapper, and the header stays free of HIP."""
    with open(os.path.join(CSRC, "ace_predict.cpp")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "ace_retry.h")) as f:
        hdr = f.read()
    assert '#include "ace_retry.h"' in src
    assert len(re.findall(r"\bretry_once_on<", src)) == 1
    assert not re.search(r"catch[^{]*\{[^}]*ACE_ERR_OOM", src)
    assert len(re.findall(r"static_pointer_cast<PredScratch>", src)) == 1
    assert not re.search(r"#include|\bhip[A-Z]", hdr)
