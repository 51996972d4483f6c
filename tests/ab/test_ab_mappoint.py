"""The packed A/B form of ComputeDistinctiveDescriptors (k_mp_distinctive_packed<G> + k_mp_distinctive_long<G>, -DORBX_AB build only):
ORBM_MP_PACKED = 8, 16 or 32 gives a MapPoint whose list has at most that many entries a group of that many lanes and leaves longer
lists to the wave kernel.  Same rows as the second reading whatever the group size is, on the lists of tests/mappoint_cases.py, whose
sizes sit on both sides of every group size."""
import pytest

pytestmark = pytest.mark.gpu
from test_gpu_mappoint import S, _Out, _enqueue, _same   # noqa: F401  (fixture + helpers)


@pytest.mark.parametrize("group", ["8", "16", "32"])
def test_packed_groups_equal_the_second_reading(pkg, S, monkeypatch, group):
    monkeypatch.setenv("ORBM_MP_PACKED", group)
    for lo, hi in ((0, None), (3, 68)):
        out = _Out(pkg, (S["M"]["nmp"] if hi is None else hi) - lo)
        assert _enqueue(S, out, lo, hi, which="d")[0] == 0, S["L"].orbm_last_error()
        S["m"].sync()
        want = {k: v[lo:hi] for k, v in S["want"].items()}
        _same(out.fetch(), want, what=("desc", "best", "med"))
