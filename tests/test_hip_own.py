"""The owning handles of azdopt_amd/csrc/hip_own.h: their failure paths, walked by tests/cpp/hip_own_check.cpp where no device is
visible (every acquisition fails there), and the rule that the library releases HIP resources in that header and nowhere else."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "azdopt_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
RELEASE_CALLS = ("hipFree(", "hipHostFree(", "hipStreamDestroy(", "hipEventDestroy(", "hipGraphExecDestroy(", "hipGraphDestroy(")
WRONG_MACHINE = 77  # hip_own_check's exit status where the mode does not fit the machine


def build_check(tmp_path):
    exe = tmp_path / "hip_own_check"
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-self-move", os.path.join(ROOT, "tests", "cpp", "hip_own_check.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    return exe


def test_every_acquisition_fails_clean_without_a_device(tmp_path):
    r = subprocess.run([str(build_check(tmp_path)), "no-device"], capture_output=True, text=True, timeout=120)
    if r.returncode == WRONG_MACHINE:
        pytest.skip("a GPU is present: tests/test_gpu_hip_own.py runs the success paths")
    assert r.returncode == 0 and r.stdout.strip() == "hip_own_check no-device: ok", (r.returncode, r.stdout, r.stderr)


def test_release_calls_stand_in_hip_own_h_and_nowhere_else():
    """hipFree, hipHostFree, hipStreamDestroy, hipEventDestroy, hipGraphExecDestroy and hipGraphDestroy are called by the handles
    alone; the one exception is capture_graph (engine_rollout.hip), whose template graph is a local with its two hipGraphDestroy calls"""
    files = sorted(glob.glob(os.path.join(CSRC, "*")))
    assert len(files) > 40 and os.path.join(CSRC, "hip_own.h") in files
    found = {}
    for path in files:
        if not os.path.isfile(path):
            continue
        text = open(path, errors="replace").read()
        for call in RELEASE_CALLS:
            n = len(re.findall(r"\b" + re.escape(call), text))
            if n:
                found[(os.path.basename(path), call)] = n
    own = {call: found.pop(("hip_own.h", call), 0) for call in RELEASE_CALLS}
    assert all(own[call] >= 1 for call in RELEASE_CALLS[:5]), own  # each handle releases what it owns
    graph = found.pop(("engine_rollout.hip", "hipGraphDestroy("), 0)
    assert found == {}, found
    assert graph + own["hipGraphDestroy("] >= 1
    if graph:
        text = open(os.path.join(CSRC, "engine_rollout.hip")).read()
        body = text[text.index("static int capture_graph("):]
        body = body[:body.index("\n}\n")]
        assert body.count("hipGraphDestroy(") == graph == 2, graph
