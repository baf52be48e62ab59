"""The loss passes write the bytes they wrote before the plain and the weighted kernels got one definition
(csrc/s2d_loss_kernels.h): gradient image and totals of every case of tests/loss_bytes_cases.py against
tests/golden/loss_bytes.json, which tools/record_loss_bytes.py recorded on an MI355X from a build of the commit before --
never from the code under test.  Equality, no tolerance: the build contracts nothing and the kernels have no atomics, so the
bytes follow from the order of the operations in the source.

The other suites hold the kernels to yardsticks (tests/test_gpu_loss.py, tests/test_gpu_pixel_weights.py); this one pins what
they leave open: a weighted pass under a plane that is not trivial, and the unweighted D-SSIM pass.
"""
import pytest

import loss_bytes_cases as LB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    cases = LB.recorded()["cases"]
    assert sorted(cases) == sorted(LB.group_key(*g) for g in LB.GROUPS)
    return cases


@pytest.mark.parametrize("scene,images,plane", LB.GROUPS, ids=[LB.group_key(*g) for g in LB.GROUPS])
def test_a_loss_pass_writes_the_recorded_bytes(recorded, scene, images, plane):
    want, got = recorded[LB.group_key(scene, images, plane)], LB.evaluate(scene, images, plane)
    assert got["image0"] == want["image0"], "the forward pass differs, not the loss: image0 is not the recorded one"
    assert sorted(got) == sorted(want) == sorted(["image0"] + [str(w) for w in LB.WEIGHTINGS])
    for w in LB.WEIGHTINGS:
        g, r = got[str(w)], want[str(w)]
        assert ("weighted" in g) == ("weighted" in r) == (plane != "none")
        assert g["grad"] == r["grad"], (scene, images, plane, w, "the gradient image")
        assert g["terms"] == r["terms"], (scene, images, plane, w, "mse, l1, dssim, total of s2d_loss_get")
        assert g.get("weighted") == r.get("weighted"), (scene, images, plane, w, "weight_sum, mse, l1, dssim, total of s2d_weighted_loss_get")
