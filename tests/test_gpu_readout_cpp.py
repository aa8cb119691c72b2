"""Runs the C++ drop-in's readout tests (tests/cpp/test_readout.cpp, built by __graft_entry__.build()) on the GPU:
PGOAgent::getTrajectoryInGlobalFrame (rounded by dpgo_hip_round_se), getPoseInGlobalFrame and
getNeighborPoseInGlobalFrame with the reference's return rules."""
import os
import subprocess

import pytest

from tests._common import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dpgo_amd", "cpp", "build", "test_readout")


@pytest.fixture(scope="module")
def cpp_output():
    assert os.path.exists(BIN), "C++ readout tests not built (run __graft_entry__.build())"
    p = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout + p.stderr


@pytest.mark.parametrize("name", ["TrajectoryInGlobalFrame", "PoseInGlobalFrame", "GlobalFrameNeedsAnchor"])
def test_cpp_readout_case(cpp_output, name):
    rc, out = cpp_output
    assert f"[PASS] {name}" in out, out[-3000:]


def test_cpp_readout_exit_status(cpp_output):
    rc, out = cpp_output
    assert rc == 0 and "ALL TESTS PASSED" in out, out[-3000:]
