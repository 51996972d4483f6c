"""The blur's forms, forced on the A/B library (ORB_LIB, see tests/test_ab_child.py) at every strip, tile and walk class of
tests/blur_cases.py: the walk on one frame and on a small batch (ORBX_BLUR_WALK=1: every chunk length 1..8, chunks of one tile
included), the one-tile form on a batch above the walk's threshold (ORBX_BLUR_WALK=0), the row-major branch of the store address
(ORBX_BLUR_ROWMAJOR, both forms) and k_blur2 (ORBX_BLUR_V2).  Same comparisons as tests/test_gpu_blur_tiles.py: every blurred
level byte for byte against the exact integer statement, results against the oracle, and the form the handle reports."""
import pytest

pytestmark = pytest.mark.gpu
import blur_cases as bc
from blur_cases import GEOMS
from test_gpu_blur_tiles import all_images, run_device, run_host


@pytest.mark.parametrize("name", list(GEOMS))
def test_walk_forced_on_one_frame_and_a_small_batch(pkg, oracle, synth, monkeypatch, name):
    monkeypatch.setenv("ORBX_BLUR_WALK", "1")
    run_device(pkg, oracle, synth, name, all_images(name), form=1)
    run_host(pkg, oracle, synth, name, all_images(name), form=1)
    run_device(pkg, oracle, synth, name, [4], form=1)
    run_host(pkg, oracle, synth, name, [5], form=1)
    run_host(pkg, oracle, synth, name, [1], form=1)


@pytest.mark.parametrize("name", list(GEOMS))
def test_one_tile_form_forced_above_the_threshold(pkg, oracle, synth, monkeypatch, name):
    tasks = bc.walk_tasks(bc.level_sizes(oracle, name))
    frames = (2048 + tasks - 1) // tasks + 1
    which = [i % GEOMS[name][4] for i in range(frames)]
    picked = [0, 1, 2, 3, 4, 5, frames // 2, frames - 2, frames - 1]
    monkeypatch.setenv("ORBX_BLUR_WALK", "0")
    run_device(pkg, oracle, synth, name, which, form=0, level_frames=picked)
    run_host(pkg, oracle, synth, name, which, form=0, level_frames=picked)


@pytest.mark.parametrize("walk", [None, "1"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_row_major_store(pkg, oracle, synth, monkeypatch, name, walk):
    monkeypatch.setenv("ORBX_BLUR_ROWMAJOR", "1")
    if walk:
        monkeypatch.setenv("ORBX_BLUR_WALK", walk)
    run_device(pkg, oracle, synth, name, all_images(name), form=1 if walk else 0)
    run_host(pkg, oracle, synth, name, all_images(name), form=1 if walk else 0)
    run_host(pkg, oracle, synth, name, [4], form=1 if walk else 0)


@pytest.mark.parametrize("name", list(GEOMS))
def test_valu_kernel(pkg, oracle, synth, monkeypatch, name):
    monkeypatch.setenv("ORBX_BLUR_V2", "1")
    run_device(pkg, oracle, synth, name, all_images(name), form=2)
    run_host(pkg, oracle, synth, name, all_images(name), form=2)
    run_host(pkg, oracle, synth, name, [4], form=2)
    run_device(pkg, oracle, synth, name, [5], form=2)
