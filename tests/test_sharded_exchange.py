"""The two rank exchanges of fastconsensus_amd/distributed.py on the CPU (gloo, world 1, 2 and 3):
_gather_rows (vote_sharded's [rows, n] blocks, cluster_match_sharded's [2, rows, K] tables) and
_sum_ranks.  Every rank checks the values it gets and counts the collectives it issues: a gather
is two all-gathers and nothing else, _sum_ranks one all-reduce per tensor, and one rank alone
issues none."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.sharded import free_port

# per-rank row counts; the last case of each world has no rows anywhere
COUNTS = {1: [(3,), (0,)], 2: [(3, 1), (0, 0)], 3: [(0, 3, 1), (0, 0, 0)]}
# (shape of a block of `rows` rows, the axis the rows lie on, counters after the row count)
USERS = {"vote": (lambda rows: (rows, 5), 0, 2), "match": (lambda rows: (2, rows, 3), 1, 3)}


def _block(user, rank, rows):
    """This rank's block: row r holds rank * 100 + r (match's second table 1000 more)."""
    shape, axis, _ = USERS[user]
    b = torch.zeros(shape(rows), dtype=torch.int32)
    for r in range(rows):
        b.select(axis, r).fill_(rank * 100 + r)
    if user == "match":
        b[1] += 1000
    return b


def _sums(user, rank, rows):
    return [rows] + [(rank + 1) * 10 ** j for j in range(1, USERS[user][2] + 1)]


class _Count:
    """Wraps dist.all_gather and dist.all_reduce with counters for the time of a `with`."""

    def __enter__(self):
        self.calls, self._orig = [], (dist.all_gather, dist.all_reduce)

        def gather(out, t, *a, **k):
            self.calls.append(("all_gather", t.dtype, t.numel()))
            return self._orig[0](out, t, *a, **k)

        def reduce(t, *a, **k):
            self.calls.append(("all_reduce", t.dtype, t.numel()))
            return self._orig[1](t, *a, **k)

        dist.all_gather, dist.all_reduce = gather, reduce
        return self

    def __exit__(self, *exc):
        dist.all_gather, dist.all_reduce = self._orig


def _check(rank, world):
    from fastconsensus_amd.distributed import _gather_rows, _sum_ranks
    for counts in COUNTS[world]:
        for user, (shape, axis, extra) in USERS.items():
            mine, sums = _block(user, rank, counts[rank]), _sums(user, rank, counts[rank])
            with _Count() as c:
                rows, tot = _gather_rows(mine, sums, "cpu", axis=axis)
            want = torch.cat([_block(user, g, counts[g]) for g in range(world)], dim=axis)
            assert rows.dtype == torch.int32 and rows.shape == want.shape and torch.equal(rows, want), (user, counts)
            assert [int(x) for x in tot] == np.sum([_sums(user, g, counts[g]) for g in range(world)], 0).tolist()
            if world == 1:
                assert c.calls == [] and rows is mine and tot is sums
            else:   # the int64 counters, then the blocks padded to the largest (one row at the least)
                pad = int(np.prod(shape(max(max(counts), 1))))
                assert c.calls == [("all_gather", torch.int64, 1 + extra), ("all_gather", torch.int32, pad)], c.calls
    a = torch.arange(4, dtype=torch.int64) + 10 * rank
    b = torch.full((2, 3), rank + 1, dtype=torch.int32)
    with _Count() as c:
        ra, rb = _sum_ranks(a, b)
    assert ra is a and rb is b
    assert torch.equal(a, world * torch.arange(4, dtype=torch.int64) + 10 * sum(range(world)))
    assert torch.equal(b, torch.full((2, 3), sum(range(1, world + 1)), dtype=torch.int32))
    assert c.calls == ([] if world == 1 else [("all_reduce", torch.int64, 4), ("all_reduce", torch.int32, 6)])


def _worker(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _check(rank, world)
    finally:
        dist.destroy_process_group()


def test_one_rank_issues_no_collective():
    assert not dist.is_initialized()
    _check(0, 1)


@pytest.mark.parametrize("world", [2, 3])
def test_exchange_over_ranks(world):
    mp.spawn(_worker, args=(world, free_port()), nprocs=world, join=True)
