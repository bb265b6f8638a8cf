"""The owning handles of azdopt_amd/csrc/hip_own.h on a device: every acquisition succeeds, memory is released exactly when its
handle lets go of it, streams, events and graph executables work through their handles (tests/cpp/hip_own_check.cpp, mode `device`)."""
import subprocess

import pytest

from test_hip_own import build_check

pytestmark = pytest.mark.gpu


def test_handles_acquire_move_and_release_on_the_device(tmp_path):
    r = subprocess.run([str(build_check(tmp_path)), "device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "hip_own_check device: ok", (r.returncode, r.stdout, r.stderr)
