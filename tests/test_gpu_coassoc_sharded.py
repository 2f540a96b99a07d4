"""coassociation_sharded over two ranks (gloo, both on the one GPU): every rank's reduced matrix
equals, bit for bit, what one engine holding all n_p labelings counts; the sharded histogram equals
that engine's fc_coassoc_hist."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import coassoc_ref as car
from tests import golden_io

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "coassoc_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("n_p,splits", [(20, ((0, 10), (10, 20))), (5, ((0, 3), (3, 5)))])
def test_two_ranks_equal_one(tmp_path, n_p, splits):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    world = len(splits)
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    labs = case.cd_batches[0][:n_p]
    rng = np.random.default_rng(n_p)
    a, b = rng.choice(case.N, 300, replace=False), rng.choice(case.N, 130, replace=False)
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0], e[:, 1])
        eng.set_labels(labs)
        exp = eng.coassociation(a, b).cpu().numpy()
        exp_sq = eng.coassociation(a).cpu().numpy()
        exp_hist = eng.coassoc_hist(a)
    assert np.array_equal(exp, car.matrix(labs, a, b)) and 0 < exp.min() + 1 <= exp.max() <= n_p
    port, prefix = _free_port(), str(tmp_path / "r")
    np.savez(prefix + "_lists.npz", a=a, b=b)
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, "-u", WORKER, "--rank", str(r), "--world", str(world), "--port", str(port),
                               "--n-p", str(n_p), "--lo", str(lo), "--hi", str(hi), "--out", prefix],
                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r, (lo, hi) in enumerate(splits)]
    try:
        for r, p in enumerate(procs):          # each child under its own limit; stop at the first failure
            out = p.communicate(timeout=120)[0].decode(errors="replace")
            assert p.returncode == 0, "rank %d exited %s:\n%s" % (r, p.returncode, out[-3000:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r in range(world):
        z = np.load(prefix + "_%d.npz" % r)
        assert z["matrix"].dtype == np.int32 and np.array_equal(z["matrix"], exp), r
        assert np.array_equal(z["square"], exp_sq), r
        assert z["hist"].dtype == np.int64 and np.array_equal(z["hist"], exp_hist), r
