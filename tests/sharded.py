"""Scaffolding of the sharded GPU tests: the parent starts one child process per rank
(`run_ranks`), each child is a worker module of this package whose `main` hands its body to
`rank_main`.  The ranks share the box's one GPU over gloo (RCCL refuses two ranks on one device).
A rank that is not reaped keeps the GPU open, so `run_ranks` never returns, or raises, with a
child alive.  A plain module: no conftest, no pytest plugin."""
import argparse
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(worker, per_rank_args, timeout):
    """Run the module tests.<worker> once per entry of `per_rank_args` (that rank's arguments after
    --rank / --world / --port), each as a child process (never an exec of this one) from the
    repository root.  Every child gets `timeout` seconds of its own; the first rank that fails
    ends the wait, with the tail of its output in the assertion; whatever is still alive then is
    killed and reaped."""
    world, port = len(per_rank_args), free_port()
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, "-u", "-m", "tests." + worker, "--rank", str(r), "--world", str(world),
                               "--port", str(port)] + [str(x) for x in args],
                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r, args in enumerate(per_rank_args)]
    try:
        for r, p in enumerate(procs):
            out = p.communicate(timeout=timeout)[0].decode(errors="replace")
            assert p.returncode == 0, "rank %d exited %s:\n%s" % (r, p.returncode, out[-3000:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()


def rank_main(body, add_arguments=None):
    """A worker's main: parse --rank / --world / --port / --out and what `add_arguments(parser)`
    adds, join the gloo group, call body(args), leave the group whatever body did."""
    ap = argparse.ArgumentParser()
    for name in ("rank", "world", "port"):
        ap.add_argument("--" + name, type=int, required=True)
    ap.add_argument("--out", required=True)
    if add_arguments:
        add_arguments(ap)
    a = ap.parse_args()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(a.port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
    try:
        body(a)
    finally:
        dist.destroy_process_group()
