"""A bounded run of the randomised GPU-vs-oracle sweep (tests/fuzz_parity.py) under `pytest -m gpu`: scenes, instance
sets, materials, debug options, depth limits, image sizes, both pipelines, both cube filters -- every draw bit-exact
in image and ray counts."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [11, 12])
def test_bounded_fuzz_parity(gpu, oracle, capi, seed):
    import fuzz_parity
    tally = {}
    assert fuzz_parity.run(100, seed, gpu, verbose=False, tally=tally) is None
    print("seed %d: %r" % (seed, tally))
    # rigid updates are among the draws, with instances that go to the identity and with hard transforms
    assert tally["draws"] == 100 and tally["animated"] > 0 and tally["with_identity"] > 0 and tally["with_hard"] > 0, tally
