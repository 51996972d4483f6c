"""facade/FrameGeometry.h's FrustumPoseRow, compiled with plain g++ against cvcompat.h on a mock Frame as a stand-alone program
(tests/frustum_pose_facade.cpp): the pose row orbm_is_in_frustum_batch_async reads, from the members Frame::isInFrustum uses.  No GPU."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_row_helper_lays_out_a_mock_frame(tmp_path):
    """FrustumPoseRow's 15 floats equal the members of a mock Frame in the documented layout: tcwRow = row-major 3x4 [mRcwx | mtcwx],
    owRow = mOwx, bit for bit (a NaN payload, -0 and a subnormal among them), from both overloads."""
    exe = str(tmp_path / "frustum_pose_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "frustum_pose_facade.cpp")])
    rng = np.random.default_rng(3)
    for trial in range(3):
        R = rng.normal(0, 1, (3, 3)).astype(np.float32); t = rng.normal(0, 2, 3).astype(np.float32); O = rng.normal(0, 2, 3).astype(np.float32)
        if trial == 1:
            R[1, 2] = np.float32(-0.0); t[0] = np.float32(1e-45); O[2] = np.float32(np.inf)
            R.view(np.uint32)[2, 0] = 0x7FC01234                             # a NaN with a payload: copied, not computed with
        args = [str(int(x)) for x in np.concatenate([R.reshape(9), t, O]).view(np.uint32)]
        res = subprocess.run([exe] + args, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        lines = res.stdout.strip().split("\n")
        assert len(lines) == 2 and lines[0] == lines[1]
        got = np.array([int(x) for x in lines[0].split()], np.uint32)
        want = np.concatenate([np.concatenate([R, t[:, None]], 1).reshape(12), O]).view(np.uint32)
        assert len(got) == 15 and np.array_equal(got, want), (trial, got, want)
