"""The other two forms of the orientation and descriptor stage, forced on the A/B library (ORB_LIB, see tests/test_ab_child.py) on the
frames of tests/orient_cases.py: k_orient_desc2 on row-major blurred levels (ORBX_BLUR_ROWMAJOR: patch rows of 40 bytes from
(cx - 18) & ~3) and k_orient_desc, one wavefront per keypoint (ORBX_OD_V1).  Same comparisons as tests/test_gpu_orient_geometry.py:
angle and descriptor of every keypoint bit for bit against the numpy statement on the device's own levels and selection, the whole
result against the oracle, and the form the handle reports."""
import pytest

pytestmark = pytest.mark.gpu
import orient_cases as oc
from test_gpu_orient_geometry import batch_specs, group, run_device, run_host, spec

FORMS = [("ORBX_BLUR_ROWMAJOR", 1), ("ORBX_OD_V1", 2)]


@pytest.mark.parametrize("switch,form", FORMS)
def test_border_and_doubled_frames(pkg, oracle, monkeypatch, switch, form):
    monkeypatch.setenv(switch, "1")
    for name in oc.BORDER + oc.DOUBLED:
        run_host(pkg, oracle, [spec(name)], form=form)
    for name in (oc.BORDER[1], oc.BORDER[3], oc.DOUBLED[1], oc.DOUBLED[3]):          # the widths whose last patch row ends in the extra tile column, as device pointers
        run_device(pkg, oracle, [spec(name)], form=form, tight=True)


@pytest.mark.parametrize("switch,form", FORMS)
def test_saturated_and_count_frames(pkg, oracle, monkeypatch, switch, form):
    monkeypatch.setenv(switch, "1")
    run_host(pkg, oracle, group("compass_and_saturated"), form=form, singly=False)
    run_host(pkg, oracle, group("counts"), form=form)
    run_device(pkg, oracle, group("counts"), form=form)


@pytest.mark.parametrize("switch,form", FORMS)
def test_batch_of_nine(pkg, oracle, monkeypatch, switch, form):
    monkeypatch.setenv(switch, "1")
    run_device(pkg, oracle, batch_specs(9), form=form)
    run_host(pkg, oracle, batch_specs(9)[1:] + batch_specs(9)[:1], form=form, singly=False)


def test_the_product_form_on_this_library(pkg, oracle):
    run_host(pkg, oracle, [spec(oc.BORDER[0])], form=0)
