"""An engine owns its device memory: whatever its calls allocate through the growable buffers,
close() gives back, to the byte (fc_device_bytes).  Every comparison is against the count taken before
the engine was created, not against zero: other tests' engines may still be alive in the process."""
import numpy as np
import pytest

from tests import golden_io

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_R = 3
ALGOS = {"louvain": 0, "lpm": 1, "leiden": 3, "infomap": 4}


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@pytest.fixture(scope="module")
def karate():
    return golden_io.load("karate_louvain_np50")


def open_engine(fcmod, case):
    e = case.edges_file
    eng = fcmod.Engine(seed=7)
    eng.load_graph(case.N, e[:, 0], e[:, 1])
    return eng


def test_full_feature_engine_returns_every_byte(fcmod, karate):
    b0 = fcmod.device_bytes()
    eng = open_engine(fcmod, karate)
    try:
        for algo in ALGOS.values():
            eng.reset_graph()
            eng.cd(algo, 0, N_R, N_R, 0)
        labels, st = eng.run(ALGOS["louvain"], N_R, 0.2, 0.02)
        assert labels.shape == (N_R, karate.N) and st["iterations"] >= 1
        assert len(eng.score_partitions()["k"]) == N_R
        cons = eng.consensus_partition()
        eng.consensus_levels()
        nodes = np.arange(karate.N, dtype=np.int32)
        assert tuple(eng.coassociation(nodes).shape) == (karate.N, karate.N)
        assert eng.cluster_consensus(cons["labels"])["n_r"] == N_R
        assert fcmod.device_bytes() > b0
    finally:
        eng.close()
    assert fcmod.device_bytes() == b0


@pytest.mark.parametrize("algo", ["leiden", "infomap"])
def test_level_state_is_freed(fcmod, karate, algo):
    """the Leiden / Infomap level buffers (Ctx::lv) go with the engine like every other buffer"""
    b0 = fcmod.device_bytes()
    with open_engine(fcmod, karate) as eng:
        eng.cd(ALGOS[algo], 0, N_R, N_R, 0)
        assert eng.get_labels(N_R).shape == (N_R, karate.N)
        assert fcmod.device_bytes() > b0
    assert fcmod.device_bytes() == b0


def test_grown_buffers_are_freed(fcmod, karate):
    from fastconsensus_amd import synth
    b0 = fcmod.device_bytes()
    with open_engine(fcmod, karate) as eng:
        eng.run(ALGOS["louvain"], N_R, 0.2, 0.02)
        small = fcmod.device_bytes()
        assert small > b0
        u, v, _ = synth.lfr(1000, 0.3, seed=3)
        eng.load_graph(1000, u, v)
        eng.run(ALGOS["louvain"], N_R, 0.2, 0.02)
        assert fcmod.device_bytes() > small      # the buffers grew on the same engine
    assert fcmod.device_bytes() == b0


def test_failed_create_holds_nothing(fcmod):
    b0 = fcmod.device_bytes()
    with pytest.raises(fcmod.FastConsensusError):
        fcmod.Engine(device=torch.cuda.device_count())
    assert fcmod.device_bytes() == b0
