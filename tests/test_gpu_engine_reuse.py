"""A used engine gives the results of a new one.

Every other bit-exact test opens an Engine, loads one graph, does one thing and closes; bench.py,
the command line and every real caller keep one engine and call it again and again.  Here a target
(one operation with a CPU reference that has no history by construction) runs after a history (what
the same Engine object did before), and is held to that reference exactly as on a new engine:
tests/reuse_cases.py holds the targets, the histories and the matrix.  No expected value comes from
a device run; the `fresh` history is the control that tells a wrong target from wrong reuse.
"""
import pytest

from tests import reuse_cases as rc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@pytest.mark.parametrize("pair", rc.MATRIX, ids=rc.pair_id)
def test_target_after_history(fcmod, pair):
    history, target = pair[0], rc.TARGET[pair[1]]
    ref = target.reference()
    with fcmod.Engine(seed=rc.create_seed(history, target.seed)) as eng:
        rc.HISTORY[history](fcmod, eng, target)
        if history in rc.NO_RELOAD:
            target.run(eng, ref, reload=False)
        else:
            target.run(eng, ref)
        if history == "timed":
            st = eng.collect_timing()          # timing was on while the target ran
            assert all(v >= 0 for k, v in st.items() if k.endswith("_ms"))


def test_chain_of_targets_forward_and_back(fcmod):
    """All targets on one engine in a fixed order, then in reverse: every target with its
    neighbours (and all that came before them) as its history."""
    with fcmod.Engine(seed=rc.RESEEDED_CREATE_SEED) as eng:
        for target in rc.TARGETS + rc.TARGETS[::-1]:
            try:
                target.run(eng, target.reference())
            except AssertionError as e:
                raise AssertionError("chain: %s failed: %s" % (target.id, e)) from e
